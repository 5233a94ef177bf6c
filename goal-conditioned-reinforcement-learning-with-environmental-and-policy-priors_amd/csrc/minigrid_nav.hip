/*
 * minigrid_nav.hip -- shortest-path distance fields and expert actions on the device (C ABI: include/minigrid_nav.h).
 *
 *   mg_nav_field_kernel    the flood runs on row bit masks: one lane per world row holds `open` (enterable cells) and
 *                          `reached` as 32-bit masks, two envs per 64-lane wavefront (lanes 0..31 / 32..63).  A step is
 *                          (reached | reached << 1 | reached >> 1 | row above | row below) & open, the neighbour rows
 *                          taken by cross-lane shuffles; one ballot per step decides "nothing new".  The loop holds no
 *                          LDS read and no barrier, and ends after at most width*height steps whatever the input.
 *                          Cells reached in step k get k written into an LDS uint16 image (a walk over the new bits of
 *                          the row); the image then leaves whole through the aligned row store (row_store.h), and one
 *                          lane per env reads the agent's cell and its four neighbours from it.
 *   mg_nav_lookup_kernel   one lane per (step, env): the cell of the position (visit_cell.h) indexes the env's field.
 *   mg_nav_moves_kernel    the set of optimal moves of every acting state of a rollout.  A workgroup owns NAV_MOVES_ELEMS
 *                          consecutive (step, env) elements: it reads their positions (and ages) coalesced, one element
 *                          per lane and round, looks the cell and its four neighbours up in the env's field (a 578-byte
 *                          row that stays in cache) and parks mask and distance in LDS; the two outputs then leave
 *                          through the aligned row store, each as the 16-byte chunks of its own alignment.
 *   mg_nav_goal_kernel     the same move sets for records that each name their own goal (hindsight records).  A workgroup
 *                          owns NAV_GOAL_ELEMS consecutive records: it parks (env, goal cell, acting cell) of each in LDS,
 *                          marks the heads (records whose (env, goal cell) differs from their predecessor's, and the
 *                          first one), compacts them into a list, and its eight half wavefronts flood one head's goal each
 *                          -- the field kernel's row masks and step, into a 2 KiB LDS image of their own -- and label the
 *                          head's run from that image.  No field reaches HBM; the outputs leave as the moves kernel's do.
 *   mg_nav_timed_field_kernel<P>  the flood over (cell, phase) of a world whose blockers move with period P: the lane of a
 *                          row holds `free` and `reached` of all P phases in registers (P is a template parameter, every
 *                          phase loop is unrolled), a round is reached[p] |= dilate(reached[p + 1 mod P]) & free[p] with
 *                          dilate = the field kernel's step plus the row itself (waiting), all phases from the masks of
 *                          the round before; one ballot per round decides "nothing new in any phase".  The image is
 *                          P * W*H distances per env in dynamic LDS, and the envs per workgroup (8, 4 or 2) follow from it.
 *                          The moves kernel serves the timed fields too (TIMED: the phase comes from the element's age).
 *   mg_nav_timed_goal_kernel<P>   the goal kernel over (cell, phase): its staging, heads and stores and the timed field
 *                          kernel's seed and round.  A record also keeps one phase byte; the
 *                          phase is no part of a run's key, one flood serves every phase.  A flooding half wavefront owns
 *                          an image of P * W*H distances in dynamic LDS, and as many halves flood at a time (8, 4, 2 or 1)
 *                          as fit 64 KiB next to the staging; the other wavefronts skip the flood loop whole.
 *   mg_nav_shape_kernel    potential-based reward shaping of a rollout (minigrid_nav.h, "Reward shaping"): the moves
 *                          kernel's shape -- a workgroup owns NAV_MOVES_ELEMS (step, env) elements, gathers the distances of
 *                          the acting and the after-step state from the env's field, parks shaped reward, shaping term and
 *                          mask in LDS and stores each as the chunks of its own alignment.  It reads `reward` for the
 *                          elements it stores only, before the barrier: shaping in place is safe.
 *   mg_nav_goal_shape_kernel   the same for records under goals of their own: the goal kernel's keys, heads and floods,
 *                          a record also keeps its after-step cell; three float operations per record.
 *   mg_nav_timed_goal_shape_kernel<P>   the same over (cell, phase): the timed goal kernel's flood loop and the goal shaping
 *                          kernel's after cells, label (nav_goal_shape_label, on the acting and the following phase's image)
 *                          and stores; its staging is larger than the move sets', so it has a flood count of its own.
 *   mg_nav_ahead_kernel    where a shortest path leads in 1..3 steps (minigrid_nav.h, "Look-ahead"): the moves kernel's shape
 *                          with a uint64 label per element (two per 16-byte chunk).  A lane walks the set bits of its
 *                          frontier word and takes nav_move_set of each cell on the env's field (nav_ahead_label, at most 19
 *                          cells); TIMED advances the phase per step.
 *   mg_nav_goal_ahead_kernel   the same labels for records under goals of their own: the goal kernel's keys, heads and
 *                          floods, nav_ahead_label on the half wavefront's image, 8 KiB of staged labels of its own.
 *   mg_nav_path_scan_kernel    path efficiency per episode (minigrid_nav.h, "Path efficiency"): a lane per env walks the
 *                          rollout in step order with four integer carries, the shaping kernel's two distances per step
 *                          gathered eight rows ahead of the chain; plain coalesced stores, no LDS.
 *   mg_nav_path_partial_kernel, mg_nav_path_finalize_kernel   the summary over the done steps, in ppo_episode_summary's
 *                          fixed order: runs per thread, lanes as a tree, wavefronts and workgroups in index order.
 *
 * Shared: nav_image_clear, nav_dilate, nav_move_set<WAIT>, nav_ahead_expand / nav_ahead_label; nav_out_span_t / nav_out_span / nav_out_store (one output of a
 * workgroup, any element type: the goal kernel and the shaping kernels; the moves and the timed goal kernel measured slower
 * on them and keep their own); nav_goal_records, _keys, _heads, _floods; nav_timed_goal_flooders(fixed, HW, P), the one
 * count of flooding halves for the three timed record launches and their queries.  On the host: nav_period_kernel (the
 * instantiation of a kernel template for a run-time period), one nav_*_ok per argument rule, and nav_record_launch_ok /
 * nav_rollout_launch_ok for the blocks of rules that the six record entry points and the four period-taking rollout entry
 * points share.  Each label kind on records still has a static and a timed kernel of its own: one body per kind on a
 * two-form world description measured slower.
 *
 * Integer work only but for the shaping term (three float32 operations, each rounded once: fp contract off) and the two
 * quotient sums of the path summary (float64, combined in a fixed order), no atomics: the results do not depend on scheduling.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "launch.h"
#include "minigrid_nav.h"
#include "row_store.h"
#include "twoarmy.h"
#include "visit_cell.h"

namespace {

constexpr int NAV_SIDE = MG_NAV_MAX_SIDE;
constexpr int NAV_CELLS = NAV_SIDE * NAV_SIDE;
constexpr int NAV_THREADS = 256;                       // 4 wavefronts
constexpr int NAV_ENVS = NAV_THREADS / NAV_SIDE;       // 8 envs per workgroup: 4096 envs are 512 workgroups
constexpr uint32_t NAV_T_DOOR = 4, NAV_T_GOAL = 8;
static_assert(NAV_SIDE == 32 && VISIT_MAX_SIDE == NAV_SIDE, "one lane per row, one mask bit per column");

// f(x, byte) for the W bytes at rowp, read as aligned words (the over-read rule of minigrid_nav.h).
template <typename F> __device__ __forceinline__ void nav_row_bytes(const uint8_t *rowp, int W, F f)
{
    const int mis = (int)((uintptr_t)rowp & 3);
    const uint32_t *wp = reinterpret_cast<const uint32_t *>(rowp - mis);
    const int nw = (mis + W + 3) >> 2;
    for (int k = 0; k < nw; ++k) {
        const uint32_t w = wp[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = 4 * k + j - mis;
            if (x >= 0 && x < W) f(x, (w >> (8 * j)) & 255u);
        }
    }
}

// the 32 ballot bits of this lane's half of the wavefront
__device__ __forceinline__ uint32_t nav_half_ballot(bool p, int half)
{
    return (uint32_t)(__ballot(p) >> (32 * half));
}

// image and the wave's own LDS traffic: orders what other lanes of the wavefront wrote before what this lane reads
__device__ __forceinline__ void nav_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Every distance of `chunks` 16-byte chunks starts unreachable: the 32 lanes of a half wavefront, then nav_wave_sync().
__device__ __forceinline__ void nav_image_clear(uint16_t *img, int r, int chunks)
{
    for (int c = r; c < chunks; c += 32)
        reinterpret_cast<uint4 *>(img)[c] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
}

// The enterable cells of the world row at type + off (state + off) as a bit mask, bit x = cell x (minigrid_nav.h:
// "Enterable cells", read by its over-read rule); goals = the cells of type 8.
__device__ __forceinline__ uint32_t nav_open_row(const uint8_t *__restrict__ type, const uint8_t *__restrict__ state,
                                                 size_t off, int W, uint32_t pass_types, int doors_open, uint32_t &goals)
{
    uint32_t open = 0, doors = 0;
    goals = 0;
    nav_row_bytes(type + off, W, [&](int x, uint32_t t) {
        if (t < 16u && ((pass_types >> t) & 1u)) {
            if (t == NAV_T_DOOR) doors |= 1u << x; else open |= 1u << x;
        }
        if (t == NAV_T_GOAL) goals |= 1u << x;
    });
    if (doors != 0u && state != nullptr && !doors_open) {
        uint32_t shut = 0;
        nav_row_bytes(state + off, W, [&](int x, uint32_t s) { if (s != 0u) shut |= 1u << x; });
        doors &= ~shut;
    }
    return open | doors;
}

// reached | its four neighbours, before the mask of enterable cells: the step of every flood (a timed one may wait)
__device__ __forceinline__ uint32_t nav_dilate(uint32_t reached, int r)
{
    const uint32_t up = __shfl_up(reached, 1, 32), dn = __shfl_down(reached, 1, 32);
    uint32_t next = reached | reached << 1 | reached >> 1;
    if (r > 0) next |= up;
    if (r < 31) next |= dn;
    return next;
}

// The flood of one half wavefront's world from the cells in `reached` (lane r holds row r; rows outside the world have
// open = 0): cells reached in step k get k written into img.  The exit ballot is wavefront-wide, so EVERY lane of the
// wavefront calls this together; a half with reached = 0 floods nothing.  At most cap steps whatever the input.
__device__ __forceinline__ void nav_flood(uint16_t *img, int r, int W, int cap, uint32_t open, uint32_t reached)
{
    uint32_t fresh = reached;
    for (int k = 0;; ++k) {
        for (uint32_t m = fresh; m != 0u; m &= m - 1u) img[r * W + (__ffs(m) - 1)] = (uint16_t)k;
        if (k >= cap) break;
        fresh = nav_dilate(reached, r) & open & ~reached;
        reached |= fresh;
        if (__ballot(fresh != 0u) == 0ull) break;                           // wavefront-uniform: both worlds are done
    }
}

// The optimal moves on cell c of a field row (minigrid_nav.h): bit k = neighbour k lies one move nearer; 0x10 on a source.
// `next` is the row the move arrives in: `row` itself for a static field, the next phase's for a timed one, where staying
// on c may be a move nearer too (WAIT: the stay bit then joins the others).
template <bool WAIT = false>
__device__ __forceinline__ uint32_t nav_move_set(const uint16_t *__restrict__ row, const uint16_t *__restrict__ next, int c,
                                                 int W, int H, uint32_t &d)
{
    d = row[c];
    if (d == 0u) return 0x10u;
    if (d == (uint32_t)MG_NAV_UNREACHABLE) return 0u;
    const int y = c / W, x = c - y * W;
    const uint32_t want = d - 1u;
    uint32_t m = 0;
    if (x > 0 && next[c - 1] == want) m |= 1u;
    if (x < W - 1 && next[c + 1] == want) m |= 2u;
    if (y > 0 && next[c - W] == want) m |= 4u;
    if (y < H - 1 && next[c + W] == want) m |= 8u;
    if (WAIT && next[c] == want) m |= 0x10u;
    return m;
}

// The phase of a clock value (minigrid_nav.h): 0 up to the episode's first step, the clock mod P after it.
__device__ __forceinline__ int nav_phase(int clock, int P) { return clock <= 0 ? 0 : clock % P; }

// One step of the look-ahead (minigrid_nav.h, "Look-ahead") from the frontier cell behind bit b of a label whose origin is
// cell c0: the bits of its successors -- the members of its move set on `row`, arriving in `next`.  A frontier lies within
// Manhattan radius 2 of c0 when it is expanded, so b - 1, b + 1, b - 7 and b + 7 stay inside the 7 x 7 window, and every
// member lies inside the world because nav_move_set puts only such cells into a set.
template <bool WAIT>
__device__ __forceinline__ uint64_t nav_ahead_expand(const uint16_t *__restrict__ row, const uint16_t *__restrict__ next,
                                                     int c0, int b, int W, int H)
{
    const int by = b / MG_NAV_AHEAD_SIDE;
    const int c = c0 + (by - 3) * W + (b - by * MG_NAV_AHEAD_SIDE - 3);
    uint32_t d;
    const uint64_t m = nav_move_set<WAIT>(row, next, c, W, H, d);
    return (m & 1u) << (b - 1) | ((m >> 1) & 1u) << (b + 1) | ((m >> 2) & 1u) << (b - MG_NAV_AHEAD_SIDE) |
           ((m >> 3) & 1u) << (b + MG_NAV_AHEAD_SIDE) | ((m >> 4) & 1u) << b;
}

// The look-ahead label of the acting state (c0, ph) in the P fields at f, `stride` elements apart (P = 1: one field), d = its
// distance.  All members of a frontier share one distance, max(d - j, 0): after min(steps, d) expansions every member has
// ended its episode and stays.  At most `steps` rounds of at most 49 cells each, whatever the input.
template <bool WAIT>
__device__ __forceinline__ uint64_t nav_ahead_label(const uint16_t *__restrict__ f, int64_t stride, int P, int ph, int c0,
                                                    int W, int H, int steps, uint32_t &d)
{
    d = f[ph * stride + c0];
    if (d == (uint32_t)MG_NAV_UNREACHABLE) return 0ull;
    uint64_t front = 1ull << (3 * MG_NAV_AHEAD_SIDE + 3);
    const int rounds = (uint32_t)steps < d ? steps : (int)d;
    for (int j = 0; j < rounds; ++j) {
        const int nph = ph + 1 >= P ? 0 : ph + 1;
        const uint16_t *row = f + ph * stride, *next = f + nph * stride;
        uint64_t out = 0;
        for (uint64_t m = front & ((1ull << (MG_NAV_AHEAD_SIDE * MG_NAV_AHEAD_SIDE)) - 1ull); m != 0ull; m &= m - 1ull)
            out |= nav_ahead_expand<WAIT>(row, next, c0, __ffsll((unsigned long long)m) - 1, W, H);
        front = out;
        ph = nph;
    }
    return front;
}

__global__ __launch_bounds__(NAV_THREADS) void mg_nav_field_kernel(
    const uint8_t *__restrict__ type, const uint8_t *__restrict__ state, int N, int W, int H, uint32_t pass_types,
    int doors_open, const int32_t *__restrict__ goal_x, const int32_t *__restrict__ goal_y, int gstride,
    const int32_t *__restrict__ agent_x, const int32_t *__restrict__ agent_y, int astride, uint16_t *__restrict__ dist,
    int64_t pitch, int32_t *__restrict__ agent_dist, int32_t *__restrict__ agent_action, int32_t *__restrict__ error)
{
    __shared__ __attribute__((aligned(16))) uint16_t image[NAV_ENVS][NAV_CELLS];
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, r = lane & 31;
    const int slot = tid >> 5;                                              // env of the workgroup: one half wavefront
    const int e = blockIdx.x * NAV_ENVS + slot;
    const int HW = W * H;
    const bool row = e < N && r < H;                                        // this lane holds a row of the world
    uint16_t *img = image[slot];

    nav_image_clear(img, r, NAV_CELLS / 8);                                 // every cell starts unreachable
    nav_wave_sync();                                                        // before other lanes write steps into it

    uint32_t open = 0, goals = 0;
    if (row) open = nav_open_row(type, state, (size_t)e * HW + (size_t)r * W, W, pass_types, doors_open, goals);

    // sources
    int err = 0;
    uint32_t reached = 0;
    if (goal_x != nullptr) {
        const bool in_n = e < N;
        const int gx = in_n ? goal_x[(int64_t)e * gstride] : 0, gy = in_n ? goal_y[(int64_t)e * gstride] : 0;
        if (gx < 0 || gx >= W || gy < 0 || gy >= H) err = 2;
        else if (r == gy) reached = (1u << gx) & open;
    } else {
        reached = goals & open;
    }
    const uint32_t sourced = nav_half_ballot(reached != 0u, half);         // every lane votes: err may differ per env
    if (err == 0 && sourced == 0u) err = 1;

    nav_flood(img, r, W, HW, open, reached);
    nav_wave_sync();

    if (e >= N) return;                                                     // a whole half wavefront at once
    if ((agent_dist != nullptr || agent_action != nullptr || (error != nullptr && agent_x != nullptr)) && r == 0) {
        const int ax = agent_x[(int64_t)e * astride], ay = agent_y[(int64_t)e * astride];
        uint32_t d = MG_NAV_UNREACHABLE, m = 0;
        if (ax >= 0 && ax < W && ay >= 0 && ay < H) m = nav_move_set(img, img, ay * W + ax, W, H, d);
        else if (err == 0) err = 3;
        if (agent_dist) agent_dist[e] = (int)d;                             // the lowest move: left, right, up, down
        if (agent_action) agent_action[e] = m == 0u ? MG_NAV_ACTION_NONE : m == 0x10u ? MG_NAV_ACTION_STAY : __ffs(m) - 1;
    }
    if (error != nullptr && r == 0) error[e] = err;
    if (dist != nullptr) {
        uint16_t *ob = dist + (int64_t)e * pitch;
        const int chunks = mg_row_chunks_at<int>(mg_row_misalign(ob, 8), HW, 8);
        for (int c = r; c < chunks; c += 32)
            mg_row_store(ob, HW, c, [&](int q) -> uint16_t { return img[q]; });
    }
}

constexpr int NAV_LOOKUP_THREADS = 256;

__global__ __launch_bounds__(NAV_LOOKUP_THREADS) void mg_nav_lookup_kernel(const uint16_t *__restrict__ dist, int64_t pitch,
                                                                           int N, int W, int H,
                                                                           const float2 *__restrict__ pos, int64_t M,
                                                                           uint16_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * NAV_LOOKUP_THREADS + threadIdx.x;
    if (i >= M) return;
    const int n = (int)(i % N);
    const float2 p = pos[i];
    const int c = visit_cell(p.x, p.y, W, H);
    out[i] = c < W * H ? dist[(int64_t)n * pitch + c] : (uint16_t)MG_NAV_UNREACHABLE;
}

// ------------------------------------------------------------------ optimal-move sets of a rollout's acting states
constexpr int NAV_MOVES_THREADS = 256;
constexpr int NAV_MOVES_ELEMS = 2048;                  // elements per workgroup: 4096 x 128 are 256 workgroups
constexpr int NAV_MOVES_ROUNDS = (NAV_MOVES_ELEMS + 16 + NAV_MOVES_THREADS - 1) / NAV_MOVES_THREADS;
static_assert(NAV_MOVES_ELEMS % 16 == 0, "whole chunks of both outputs");

// One output of a workgroup that owns `elems` consecutive elements (E per 16-byte chunk): its chunks of it, the elements
// they hold -- within [elems * b - 15, elems * (b + 1)) and inside [0, M) -- and the element of slot 0 of its LDS staging.
struct nav_out_span_t {
    mg_row_span_t<int64_t> k;
    int64_t base;
    bool has;                                           // the output is given and the workgroup holds some of it
    __device__ __forceinline__ bool holds(int64_t p) const { return has && p >= k.p_lo && p < k.p_hi; }
};
template <typename T> __device__ __forceinline__ nav_out_span_t nav_out_span(const T *out, int64_t M, int64_t b, int elems)
{
    constexpr int E = 16 / sizeof(T);
    const int s = out ? mg_row_misalign(out, E) : 0;
    nav_out_span_t o;
    o.k = mg_row_span<int64_t>(s, M, b, elems / E, E);
    o.base = E * o.k.c0 - s;
    o.has = out != nullptr && o.k.c0 < o.k.c1;
    return o;
}
// the staged elements leave through the aligned row store; after a __syncthreads()
template <typename T> __device__ __forceinline__ void nav_out_store(T *__restrict__ out, int64_t M, const nav_out_span_t &o,
                                                                    const T *staged, int threads)
{
    if (!o.has) return;
    for (int64_t c = o.k.c0 + threadIdx.x; c < o.k.c1; c += threads)
        mg_row_store(out, M, c, [&](int64_t p) { return *reinterpret_cast<const uint4 *>(staged + (int)(p - o.base)); },
                     [&](int64_t q) { return staged[(int)(q - o.base)]; });
}

// TIMED: dist holds P fields per env, age is given and is the clock of the element (mg_nav_timed_moves).
template <bool TIMED> __global__ __launch_bounds__(NAV_MOVES_THREADS) void mg_nav_moves_kernel(
    const uint16_t *__restrict__ dist, int64_t pitch, int P, int N, int W, int H, const float2 *__restrict__ pos,
    const int32_t *__restrict__ age, const float *__restrict__ init_pos, int64_t M, uint8_t *__restrict__ moves,
    uint16_t *__restrict__ acting_dist)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_moves[NAV_MOVES_ELEMS];
    __shared__ __attribute__((aligned(16))) uint16_t s_dist[NAV_MOVES_ELEMS];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    // its two spans by hand, as before nav_out_span_t: on that the launch measured 0.9 % slower
    const int sm = mg_row_misalign(moves, 16), sd = acting_dist ? mg_row_misalign(acting_dist, 8) : 0;
    const mg_row_span_t<int64_t> km = mg_row_span<int64_t>(sm, M, b, NAV_MOVES_ELEMS / 16, 16);
    const mg_row_span_t<int64_t> kd = mg_row_span<int64_t>(sd, M, b, NAV_MOVES_ELEMS / 8, 8);
    const int64_t bm = 16 * km.c0 - sm, bd = 8 * kd.c0 - sd;               // position of LDS slot 0 of either image
    const int HW = W * H;
    float2 init = make_float2(0.f, 0.f);
    if (age != nullptr) init = make_float2(init_pos[0], init_pos[1]);

    const int64_t p0 = (int64_t)NAV_MOVES_ELEMS * b - 16;
#pragma unroll 1
    for (int k = 0; k < NAV_MOVES_ROUNDS; ++k) {
        const int64_t p = p0 + k * NAV_MOVES_THREADS + tid;
        const bool in_m = p >= km.p_lo && p < km.p_hi;
        const bool in_d = acting_dist != nullptr && p >= kd.p_lo && p < kd.p_hi;
        if (!(in_m || in_d)) continue;                                      // both spans lie inside [0, M)
        float2 q = pos[p];
        const int clock = age != nullptr ? age[p] : 1;
        if (clock <= 0) q = init;
        const int c = visit_cell(q.x, q.y, W, H);
        uint32_t d = MG_NAV_UNREACHABLE, m = 0;
        if (TIMED) {
            const int ph = nav_phase(clock, P);
            const uint16_t *f = dist + (int64_t)(p % N) * P * pitch;
            if (c < HW) m = nav_move_set<true>(f + ph * pitch, f + (ph + 1 == P ? 0 : ph + 1) * pitch, c, W, H, d);
        } else if (c < HW) {
            const uint16_t *f = dist + (int64_t)(p % N) * pitch;
            m = nav_move_set(f, f, c, W, H, d);
        }
        if (in_m) s_moves[(int)(p - bm)] = (uint8_t)m;
        if (in_d) s_dist[(int)(p - bd)] = (uint16_t)d;
    }
    __syncthreads();

    for (int64_t c = km.c0 + tid; c < km.c1; c += NAV_MOVES_THREADS)
        mg_row_store(moves, M, c, [&](int64_t p) { return *reinterpret_cast<const uint4 *>(s_moves + (int)(p - bm)); },
                     [&](int64_t q) { return s_moves[(int)(q - bm)]; });
    if (acting_dist != nullptr)
        for (int64_t c = kd.c0 + tid; c < kd.c1; c += NAV_MOVES_THREADS)
            mg_row_store(acting_dist, M, c,
                         [&](int64_t p) { return *reinterpret_cast<const uint4 *>(s_dist + (int)(p - bd)); },
                         [&](int64_t q) { return s_dist[(int)(q - bd)]; });
}

// ------------------------------------------------------------------ look-ahead labels of a rollout's acting states
// The moves kernel's shape with a uint64 label per element: two labels per 16-byte chunk.
template <bool TIMED> __global__ __launch_bounds__(NAV_MOVES_THREADS) void mg_nav_ahead_kernel(
    const uint16_t *__restrict__ dist, int64_t pitch, int P, int N, int W, int H, const float2 *__restrict__ pos,
    const int32_t *__restrict__ age, const float *__restrict__ init_pos, int64_t M, int steps,
    unsigned long long *__restrict__ ahead, uint16_t *__restrict__ acting_dist)
{
    __shared__ __attribute__((aligned(16))) unsigned long long s_ahead[NAV_MOVES_ELEMS];
    __shared__ __attribute__((aligned(16))) uint16_t s_dist[NAV_MOVES_ELEMS];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const nav_out_span_t sa = nav_out_span(ahead, M, b, NAV_MOVES_ELEMS);
    const nav_out_span_t sd = nav_out_span(acting_dist, M, b, NAV_MOVES_ELEMS);
    const int HW = W * H;
    float2 init = make_float2(0.f, 0.f);
    if (age != nullptr) init = make_float2(init_pos[0], init_pos[1]);

    const int64_t p0 = (int64_t)NAV_MOVES_ELEMS * b - 16;
#pragma unroll 1
    for (int k = 0; k < NAV_MOVES_ROUNDS; ++k) {
        const int64_t p = p0 + k * NAV_MOVES_THREADS + tid;
        const bool in_a = sa.holds(p), in_d = sd.holds(p);
        if (!(in_a || in_d)) continue;                                      // both spans lie inside [0, M)
        float2 q = pos[p];
        const int clock = age != nullptr ? age[p] : 1;
        if (clock <= 0) q = init;
        const int c = visit_cell(q.x, q.y, W, H);
        uint32_t d = MG_NAV_UNREACHABLE;
        uint64_t a = 0;
        if (c < HW) {
            if (TIMED) a = nav_ahead_label<true>(dist + (int64_t)(p % N) * P * pitch, pitch, P, nav_phase(clock, P), c, W, H, steps, d);
            else a = nav_ahead_label<false>(dist + (int64_t)(p % N) * pitch, 0, 1, 0, c, W, H, steps, d);
        }
        if (in_a) s_ahead[(int)(p - sa.base)] = a;
        if (in_d) s_dist[(int)(p - sd.base)] = (uint16_t)d;
    }
    __syncthreads();
    nav_out_store(ahead, M, sa, s_ahead, NAV_MOVES_THREADS);
    nav_out_store(acting_dist, M, sd, s_dist, NAV_MOVES_THREADS);
}

// ------------------------------------------------------------------ optimal-move sets of records with goals of their own
constexpr int NAV_GOAL_THREADS = 256;
constexpr int NAV_GOAL_HALVES = NAV_GOAL_THREADS / 32;  // 8 half wavefronts, one flood each at a time
constexpr int NAV_GOAL_ELEMS = 1024;                    // records per workgroup: 500 k records are 490 workgroups
constexpr int NAV_GOAL_SLOTS = NAV_GOAL_ELEMS + 16;     // both outputs' chunks lie within [ELEMS * b - 15, ELEMS * (b + 1))
constexpr int NAV_GOAL_ROUNDS = (NAV_GOAL_SLOTS + NAV_GOAL_THREADS - 1) / NAV_GOAL_THREADS;
constexpr uint16_t NAV_NO_CELL = 0xFFFF;
static_assert(NAV_GOAL_ELEMS % 16 == 0, "whole chunks of both outputs");
static_assert(NAV_GOAL_SLOTS <= 0xFFFF, "slots are listed as uint16");

// What a workgroup keeps of its records besides the flood images: keys, heads and the labels on their way out.
struct nav_goal_stage_t {
    alignas(16) uint8_t moves[NAV_GOAL_ELEMS];
    alignas(16) uint16_t dist[NAV_GOAL_ELEMS];
    int32_t env[NAV_GOAL_SLOTS];                        // the key of a record: its env, -1 for a record without a result,
    uint16_t goal[NAV_GOAL_SLOTS];                      //   and its goal cell
    uint16_t cell[NAV_GOAL_SLOTS];                      // its acting cell, NAV_NO_CELL where the position is none
    uint16_t head[NAV_GOAL_SLOTS + 1];                  // the slots of the heads in ascending order, then the end slot
    int count[NAV_GOAL_ROUNDS][NAV_GOAL_THREADS / 64];
};

// The records of workgroup b: those that the spans of its outputs hold between them.
struct nav_goal_records_t {
    int64_t p0;                                         // record of slot 0 of the key arrays
    int slot_lo, slot_hi;                               // 0 < slot_lo <= slot_hi <= SLOTS, or both 0: no record
};
template <typename... Spans>
__device__ __forceinline__ nav_goal_records_t nav_goal_records(int64_t M, int64_t b, const Spans &...spans)
{
    nav_goal_records_t g;
    g.p0 = (int64_t)NAV_GOAL_ELEMS * b - 16;
    int64_t lo = M, hi = 0;
    auto join = [&](const nav_out_span_t &o) {
        if (o.has) { lo = lo < o.k.p_lo ? lo : o.k.p_lo; hi = hi > o.k.p_hi ? hi : o.k.p_hi; }
    };
    (join(spans), ...);
    // a workgroup that holds no span (the last one may) has no slots
    g.slot_lo = lo < hi ? (int)(lo - g.p0) : 0;
    g.slot_hi = lo < hi ? (int)(hi - g.p0) : 0;
    return g;
}

// Keys and acting cells: every global read of a record happens here, one record per lane and round; __syncthreads() after.
// TIMED: age is given and is the record's clock too; its phase goes into s_phase (0 for a record without a result).
// G: the workgroup's records (p0, slot_lo, slot_hi).  more(i, p, at): what else a kernel keeps of the record p in slot i,
// at = its element t * N + n, or -1 for a record without a result.
template <bool TIMED, typename G, typename More> __device__ __forceinline__ void nav_goal_keys(
    nav_goal_stage_t &st, uint8_t *s_phase, const G &g, int N, int W, int H, int P,
    const int32_t *__restrict__ rec_t, const int32_t *__restrict__ rec_n, const float *__restrict__ rec_goal,
    const float2 *__restrict__ pos, const int32_t *__restrict__ age, const float *__restrict__ init_pos, int T, More more)
{
    const int tid = threadIdx.x, HW = W * H;
    float2 init = make_float2(0.f, 0.f);
    if (age != nullptr) init = make_float2(init_pos[0], init_pos[1]);
#pragma unroll 1
    for (int k = 0; k < NAV_GOAL_ROUNDS; ++k) {
        const int i = k * NAV_GOAL_THREADS + tid;
        if (i < g.slot_lo || i >= g.slot_hi) continue;
        const int64_t p = g.p0 + i;
        const int t = rec_t[p], n = rec_n[p];
        const int gc = visit_cell(rec_goal[2 * p], rec_goal[2 * p + 1], W, H);   // (y, x); 4-byte aligned: two loads
        int env = -1, ac = NAV_NO_CELL, ph = 0;
        int64_t at = -1;
        if (t >= 0 && t < T && n >= 0 && n < N && gc < HW) {
            at = (int64_t)t * N + n;
            float2 q = pos[at];
            const int clock = age != nullptr ? age[at] : 1;
            if (clock <= 0) q = init;
            const int c = visit_cell(q.x, q.y, W, H);
            env = n;
            if (c < HW) ac = c;
            if (TIMED) ph = nav_phase(clock, P);
        }
        st.env[i] = env;
        st.goal[i] = (uint16_t)gc;
        st.cell[i] = (uint16_t)ac;
        if (TIMED) s_phase[i] = (uint8_t)ph;
        more(i, p, at);
    }
    __syncthreads();
}

__device__ __forceinline__ void nav_goal_no_more(int, int64_t, int64_t) {}

// Heads (records whose (env, goal cell) differs from their predecessor's, and the first one), counted per wavefront and
// round (the round's ballot stays in registers), then listed in st.head in ascending order; -> their number.
template <typename G> __device__ __forceinline__ int nav_goal_heads(nav_goal_stage_t &st, const G &g)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long heads[NAV_GOAL_ROUNDS];
#pragma unroll
    for (int k = 0; k < NAV_GOAL_ROUNDS; ++k) {
        const int i = k * NAV_GOAL_THREADS + tid;
        const bool hd = i >= g.slot_lo && i < g.slot_hi &&
                        (i == g.slot_lo || st.env[i] != st.env[i - 1] || st.goal[i] != st.goal[i - 1]);
        heads[k] = __ballot(hd);
        if (lane == 0) st.count[k][wave] = __popcll(heads[k]);
    }
    __syncthreads();
    int n_heads = 0;
#pragma unroll
    for (int k = 0; k < NAV_GOAL_ROUNDS; ++k) {
        const int i = k * NAV_GOAL_THREADS + tid;
        const unsigned long long hb = heads[k];
        const bool hd = (hb >> lane) & 1ull;
        int before = n_heads;
        for (int w = 0; w < NAV_GOAL_THREADS / 64; ++w) {
            const int cnt = st.count[k][w];
            if (w < wave) before += cnt;
            n_heads += cnt;
        }
        if (hd) st.head[before + __popcll(hb & ((1ull << lane) - 1ull))] = (uint16_t)i;
    }
    if (tid == 0) st.head[n_heads] = (uint16_t)g.slot_hi;
    __syncthreads();
    return n_heads;
}

// the label of record p, parked for the stores of `moves` (sm) and `acting_dist` (sd)
__device__ __forceinline__ void nav_goal_label(nav_goal_stage_t &st, const nav_out_span_t &sm, const nav_out_span_t &sd,
                                               int64_t p, uint32_t m, uint32_t d)
{
    if (sm.holds(p)) st.moves[(int)(p - sm.base)] = (uint8_t)m;
    if (sd.holds(p)) st.dist[(int)(p - sd.base)] = (uint16_t)d;
}

// One head per half wavefront and round: flood its goal into the half's image `img`, then label(i, img, ok) every record
// (slot i) of its run; ok = the run has a result at all.  Both halves of a wavefront go round together, and EVERY lane of
// the workgroup calls this.  What label() parks in LDS is ordered before the next flood; __syncthreads() before the stores.
template <typename Label> __device__ __forceinline__ void nav_goal_floods(
    const nav_goal_stage_t &st, uint16_t *img, int n_heads, const uint8_t *__restrict__ type,
    const uint8_t *__restrict__ state, int W, int H, uint32_t pass_types, int doors_open, Label label)
{
    const int tid = threadIdx.x, r = tid & 31, half = tid >> 5;
    const int HW = W * H;
    const int per = (n_heads + NAV_GOAL_HALVES - 1) / NAV_GOAL_HALVES;
    const int j_end = (half + 1) * per < n_heads ? (half + 1) * per : n_heads;
    int cur_env = -1;
    uint32_t open = 0;
#pragma unroll 1
    for (int it = 0; it < per; ++it) {
        const int j = half * per + it;
        const bool mine = j < j_end;
        const int s0 = mine ? st.head[j] : 0, s1 = mine ? st.head[j + 1] : 0;
        const int env = mine ? st.env[s0] : -1;
        uint32_t reached = 0;
        if (env >= 0) {
            if (env != cur_env) {                                           // the previous head's world stays in `open`
                uint32_t goals;
                open = r < H ? nav_open_row(type, state, (size_t)env * HW + (size_t)r * W, W, pass_types, doors_open, goals)
                             : 0u;
                cur_env = env;
            }
            const int gc = st.goal[s0], gy = gc / W;
            if (r == gy) reached = (1u << (gc - gy * W)) & open;
            nav_image_clear(img, r, NAV_CELLS / 8);
        }
        nav_wave_sync();                                                    // before other lanes write steps into it
        nav_flood(img, r, W, HW, env >= 0 ? open : 0u, reached);
        nav_wave_sync();
        for (int i = s0 + r; i < s1; i += 32) label(i, img, env >= 0);
        nav_wave_sync();                                                    // the labels are read before the image is reset
    }
}

__global__ __launch_bounds__(NAV_GOAL_THREADS) void mg_nav_goal_kernel(
    const uint8_t *__restrict__ type, const uint8_t *__restrict__ state, int N, int W, int H, uint32_t pass_types,
    int doors_open, const int32_t *__restrict__ rec_t, const int32_t *__restrict__ rec_n,
    const float *__restrict__ rec_goal, int64_t M, const float2 *__restrict__ pos, const int32_t *__restrict__ age,
    const float *__restrict__ init_pos, int T, uint8_t *__restrict__ moves, uint16_t *__restrict__ acting_dist)
{
    __shared__ __attribute__((aligned(16))) uint16_t image[NAV_GOAL_HALVES][NAV_CELLS];
    __shared__ nav_goal_stage_t st;
    const nav_out_span_t sm = nav_out_span(moves, M, blockIdx.x, NAV_GOAL_ELEMS);
    const nav_out_span_t sd = nav_out_span(acting_dist, M, blockIdx.x, NAV_GOAL_ELEMS);
    const nav_goal_records_t g = nav_goal_records(M, blockIdx.x, sm, sd);

    nav_goal_keys<false>(st, nullptr, g, N, W, H, 1, rec_t, rec_n, rec_goal, pos, age, init_pos, T, nav_goal_no_more);
    const int n_heads = nav_goal_heads(st, g);
    nav_goal_floods(st, image[threadIdx.x >> 5], n_heads, type, state, W, H, pass_types, doors_open,
                    [&](int i, const uint16_t *img, bool ok) {
                        const int c = st.cell[i];
                        uint32_t d = MG_NAV_UNREACHABLE, m = 0;
                        if (ok && c != NAV_NO_CELL) m = nav_move_set(img, img, c, W, H, d);
                        nav_goal_label(st, sm, sd, g.p0 + i, m, d);
                    });
    __syncthreads();
    nav_out_store(moves, M, sm, st.moves, NAV_GOAL_THREADS);
    nav_out_store(acting_dist, M, sd, st.dist, NAV_GOAL_THREADS);
}

// ------------------------------------------------------------------ look-ahead labels of records with goals of their own
// The goal kernel with a uint64 label per record: the labels on their way out have a struct of their own, so that
// nav_goal_stage_t (from which mg_nav_timed_goal_moves sizes its floods) stays as it is.
struct nav_goal_ahead_stage_t {
    alignas(16) unsigned long long ahead[NAV_GOAL_ELEMS];
};
static_assert(sizeof(nav_goal_stage_t) + sizeof(nav_goal_ahead_stage_t) + NAV_GOAL_HALVES * NAV_CELLS * sizeof(uint16_t) + 64
                  <= 64 * 1024, "the staging of a look-ahead workgroup fits 64 KiB next to its 8 images");

__global__ __launch_bounds__(NAV_GOAL_THREADS) void mg_nav_goal_ahead_kernel(
    const uint8_t *__restrict__ type, const uint8_t *__restrict__ state, int N, int W, int H, uint32_t pass_types,
    int doors_open, const int32_t *__restrict__ rec_t, const int32_t *__restrict__ rec_n,
    const float *__restrict__ rec_goal, int64_t M, const float2 *__restrict__ pos, const int32_t *__restrict__ age,
    const float *__restrict__ init_pos, int T, int steps, unsigned long long *__restrict__ ahead,
    uint16_t *__restrict__ acting_dist)
{
    __shared__ __attribute__((aligned(16))) uint16_t image[NAV_GOAL_HALVES][NAV_CELLS];
    __shared__ nav_goal_stage_t st;
    __shared__ nav_goal_ahead_stage_t sh;
    const nav_out_span_t sa = nav_out_span(ahead, M, blockIdx.x, NAV_GOAL_ELEMS);
    const nav_out_span_t sd = nav_out_span(acting_dist, M, blockIdx.x, NAV_GOAL_ELEMS);
    const nav_goal_records_t g = nav_goal_records(M, blockIdx.x, sa, sd);

    nav_goal_keys<false>(st, nullptr, g, N, W, H, 1, rec_t, rec_n, rec_goal, pos, age, init_pos, T, nav_goal_no_more);
    const int n_heads = nav_goal_heads(st, g);
    nav_goal_floods(st, image[threadIdx.x >> 5], n_heads, type, state, W, H, pass_types, doors_open,
                    [&](int i, const uint16_t *img, bool ok) {
                        const int c = st.cell[i];
                        const int64_t p = g.p0 + i;
                        uint32_t d = MG_NAV_UNREACHABLE;
                        uint64_t a = 0;
                        if (ok && c != NAV_NO_CELL) a = nav_ahead_label<false>(img, 0, 1, 0, c, W, H, steps, d);
                        if (sa.holds(p)) sh.ahead[(int)(p - sa.base)] = a;
                        if (sd.holds(p)) st.dist[(int)(p - sd.base)] = (uint16_t)d;
                    });
    __syncthreads();
    nav_out_store(ahead, M, sa, sh.ahead, NAV_GOAL_THREADS);
    nav_out_store(acting_dist, M, sd, st.dist, NAV_GOAL_THREADS);
}

// ------------------------------------------------------------------ time-expanded fields: blockers that move with period P
constexpr int NAV_MAX_PERIOD = MG_NAV_MAX_PERIOD;
constexpr int NAV_TIMED_LDS = 48 * 1024;               // the image of a workgroup where 4 or 8 envs share one: 3 fit on a CU
// uint16 elements of one phase's image: whole 16-byte chunks, so that every env's images start on one
__host__ __device__ inline int nav_timed_cells(int HW) { return (HW + 7) & ~7; }
// the dynamic LDS of a launch: `images` times P phase images
inline size_t nav_timed_bytes(int images, int HW, int P) { return (size_t)images * P * nav_timed_cells(HW) * sizeof(uint16_t); }
// Envs of a workgroup: 8 as in the field kernel while their images fit NAV_TIMED_LDS, else 4, else 2 (one wavefront; at
// P = 16 and 32 x 32 cells that is 64 KiB, the most a launch asks for).
inline int nav_timed_envs(int HW, int P)
{
    int envs = NAV_ENVS;
    while (envs > 2 && nav_timed_bytes(envs, HW, P) > (size_t)NAV_TIMED_LDS) envs >>= 1;
    return envs;
}

// The sources of a timed flood: the cells of `src` in every phase in which they are free, at distance 0.  -> the row's
// sources of any phase.
template <int P> __device__ __forceinline__ uint32_t nav_timed_seed(uint16_t *img, int cells, int r, int W, uint32_t src,
                                                                    const uint32_t (&fr)[P], uint32_t (&reached)[P])
{
    uint32_t any = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        reached[p] = src & fr[p];
        any |= reached[p];
        for (uint32_t m = reached[p]; m != 0u; m &= m - 1u) img[p * cells + r * W + (__ffs(m) - 1)] = 0;
    }
    return any;
}

// Round k of a timed flood: the states k transitions from a source.  Every phase reads its successor's mask of the round
// before: phase p is updated before phase p + 1, and the last phase reads the dilation of phase 0 taken first.
// -> something was new in some world of the wavefront (one ballot: EVERY lane of the wavefront calls this together).
template <int P> __device__ __forceinline__ bool nav_timed_round(uint16_t *img, int cells, int r, int W, int k,
                                                                 const uint32_t (&fr)[P], uint32_t (&reached)[P])
{
    const uint32_t d0 = nav_dilate(reached[0], r);
    uint32_t any = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const uint32_t d = p + 1 < P ? nav_dilate(reached[p + 1 < P ? p + 1 : 0], r) : d0;
        const uint32_t fresh = d & fr[p] & ~reached[p];
        reached[p] |= fresh;
        any |= fresh;
        for (uint32_t m = fresh; m != 0u; m &= m - 1u) img[p * cells + r * W + (__ffs(m) - 1)] = (uint16_t)k;
    }
    return __ballot(any != 0u) != 0ull;
}

// The rounds of one half wavefront's world from the seeded masks, at most cap of them whatever the input.  A half with
// reached = 0 in every phase floods nothing, whatever its fr.
template <int P> __device__ __forceinline__ void nav_timed_flood(uint16_t *img, int cells, int r, int W, int cap,
                                                                 const uint32_t (&fr)[P], uint32_t (&reached)[P])
{
    for (int k = 1; k <= cap; ++k)
        if (!nav_timed_round<P>(img, cells, r, W, k, fr, reached)) break;    // wavefront-uniform: both worlds are done
}

template <int P> __global__ __launch_bounds__(NAV_THREADS) void mg_nav_timed_field_kernel(
    const uint8_t *__restrict__ type, const uint8_t *__restrict__ state, int N, int W, int H, uint32_t pass_types,
    int doors_open, const uint32_t *__restrict__ blocked, int64_t bstride, const int32_t *__restrict__ goal_x,
    const int32_t *__restrict__ goal_y, int gstride, const int32_t *__restrict__ agent_x,
    const int32_t *__restrict__ agent_y, const int32_t *__restrict__ agent_clock, int astride,
    uint16_t *__restrict__ dist, int64_t pitch, int32_t *__restrict__ agent_dist, int32_t *__restrict__ agent_action,
    int32_t *__restrict__ error)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t timed_image[];  // [envs of the workgroup][P][cells]
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, r = lane & 31;
    const int slot = tid >> 5;                                              // env of the workgroup: one half wavefront
    const int e = blockIdx.x * (int)(blockDim.x >> 5) + slot;
    const int HW = W * H, cells = nav_timed_cells(HW);
    const bool row = e < N && r < H;                                        // this lane holds a row of the world
    uint16_t *img = timed_image + (size_t)slot * P * cells;

    nav_image_clear(img, r, P * cells / 8);                                 // every state starts unreachable
    nav_wave_sync();                                                        // before other lanes write rounds into it

    uint32_t open = 0, goals = 0;
    if (row) open = nav_open_row(type, state, (size_t)e * HW + (size_t)r * W, W, pass_types, doors_open, goals);
    uint32_t fr[P], reached[P];                                             // free and reached cells of the row per phase
#pragma unroll
    for (int p = 0; p < P; ++p) fr[p] = row ? open & ~blocked[(int64_t)e * bstride + p * H + r] : 0u;

    // sources: the same cells in every phase, each where it is free
    int err = 0;
    uint32_t src = 0;
    if (goal_x != nullptr) {
        const bool in_n = e < N;
        const int gx = in_n ? goal_x[(int64_t)e * gstride] : 0, gy = in_n ? goal_y[(int64_t)e * gstride] : 0;
        if (gx < 0 || gx >= W || gy < 0 || gy >= H) err = 2;
        else if (r == gy) src = 1u << gx;
    } else {
        src = goals;
    }
    const uint32_t any = nav_timed_seed<P>(img, cells, r, W, src, fr, reached);
    const uint32_t sourced = nav_half_ballot(any != 0u, half);             // every lane votes: err may differ per env
    if (err == 0 && sourced == 0u) err = 1;

    nav_timed_flood<P>(img, cells, r, W, HW * P, fr, reached);
    nav_wave_sync();

    if (e >= N) return;                                                     // a whole half wavefront at once
    // The agent, as this kernel had it before nav_move_set: on that and on shared helpers it measured 0.6 % slower.
    if (agent_dist != nullptr || agent_action != nullptr || (error != nullptr && agent_x != nullptr)) {
        if (r == 0) {
            const int ax = agent_x[(int64_t)e * astride], ay = agent_y[(int64_t)e * astride];
            int d = MG_NAV_UNREACHABLE, a = MG_NAV_ACTION_NONE;
            if (ax < 0 || ax >= W || ay < 0 || ay >= H) {
                if (err == 0) err = 3;
            } else {
                const int ph = nav_phase(agent_clock != nullptr ? agent_clock[(int64_t)e * astride] : 0, P);
                const uint16_t *next = img + (ph + 1 == P ? 0 : ph + 1) * cells;
                const int c = ay * W + ax;
                d = img[ph * cells + c];
                if (d == 0) a = MG_NAV_ACTION_STAY;
                else if (d != MG_NAV_UNREACHABLE) {
                    const int want = d - 1;
                    if (ax > 0 && next[c - 1] == want) a = 0;
                    else if (ax < W - 1 && next[c + 1] == want) a = 1;
                    else if (ay > 0 && next[c - W] == want) a = 2;
                    else if (ay < H - 1 && next[c + W] == want) a = 3;
                    else a = MG_NAV_ACTION_STAY;                            // waiting is the only optimal move
                }
            }
            if (agent_dist) agent_dist[e] = d;
            if (agent_action) agent_action[e] = a;
        }
    }
    if (error != nullptr && r == 0) error[e] = err;
    if (dist != nullptr) {
        for (int p = 0; p < P; ++p) {
            uint16_t *ob = dist + ((int64_t)e * P + p) * pitch;
            const uint16_t *ip = img + p * cells;
            const int chunks = mg_row_chunks_at<int>(mg_row_misalign(ob, 8), HW, 8);
            for (int c = r; c < chunks; c += 32)
                mg_row_store(ob, HW, c, [&](int q) -> uint16_t { return ip[q]; });
        }
    }
}

// kernel(std::integral_constant<int, P>) -> the instantiation of a kernel template for period P: the one of a run-time period
template <typename F, int... Ps> auto nav_period_kernel(int period, F kernel, std::integer_sequence<int, Ps...>)
{
    const decltype(kernel(std::integral_constant<int, 1>{})) of[] = {kernel(std::integral_constant<int, Ps + 1>{})...};
    return of[period - 1];
}
template <typename F> auto nav_period_kernel(int period, F kernel)
{
    return nav_period_kernel(period, kernel, std::make_integer_sequence<int, NAV_MAX_PERIOD>{});
}

// ------------------------------------------------------------------ timed move sets of records with goals of their own
// mg_nav_goal_kernel over (cell, phase): the same staging, heads and stores; a flooding half wavefront owns an image of
// P * cells distances in dynamic LDS, and `flooders` of the 8 halves flood at a time: 8, 4, 2 or 1, as many as fit 64 KiB next
// to the `fixed` bytes of the kernel that asks (nav_timed_goal_flooders; the shaping and the look-ahead staging are larger).
// The phase is no part of a run's key: one flood serves the records of every phase.
inline int nav_timed_goal_flooders(size_t fixed, int HW, int P)   // fixed: the kernel's static LDS and what aligning it may cost
{
    int f = NAV_GOAL_HALVES;
    while (f > 1 && fixed + nav_timed_bytes(f, HW, P) > (size_t)64 * 1024) f >>= 1;
    return f;
}
constexpr size_t NAV_TIMED_GOAL_LDS = sizeof(nav_goal_stage_t) + NAV_GOAL_SLOTS + 64;   // of the move sets: staging and phase bytes
static_assert(NAV_TIMED_GOAL_LDS + NAV_MAX_PERIOD * NAV_CELLS * sizeof(uint16_t) <= 64 * 1024,
              "one image of the longest period and the largest world fits next to the staging");

// The flood loop of a timed goal kernel, written once (as nav_goal_floods is for the static ones): one head per flooding
// half wavefront and round -- the head's world (kept in `fr` across heads of one env), image reset, seed, flood -- then
// label(i, img, ok) for every record (slot i) of its run; img = the half's P images of `cells` distances each, ok = the run
// has a result at all.  Whole wavefronts enter or skip the loop: one goes round when its first half floods, an idle second
// half beside it with empty masks (the ballot of a round is wavefront-wide); the trip count is the workgroup's, and no
// workgroup barrier stands inside the loop.  EVERY lane of the workgroup calls this; what label() parks in LDS is ordered
// before the next flood; __syncthreads() before the stores.
template <int P, typename Label> __device__ __forceinline__ void nav_timed_goal_floods(
    const nav_goal_stage_t &st, uint16_t *images, int n_heads, int flooders, const uint8_t *__restrict__ type,
    const uint8_t *__restrict__ state, int W, int H, uint32_t pass_types, int doors_open,
    const uint32_t *__restrict__ blocked, int64_t bstride, Label label)
{
    const int tid = threadIdx.x, r = tid & 31, half = tid >> 5;
    const int HW = W * H, cells = nav_timed_cells(HW);
    const bool floods = half < flooders;
    if ((half & ~1) < flooders) {
        uint16_t *img = images + (size_t)(floods ? half : 0) * P * cells;
        const int per = (n_heads + flooders - 1) / flooders;
        const int j_end = !floods ? 0 : (half + 1) * per < n_heads ? (half + 1) * per : n_heads;
        int cur_env = -1;
        uint32_t fr[P], reached[P];                                         // free and reached cells of the row per phase
#pragma unroll
        for (int p = 0; p < P; ++p) fr[p] = 0u;
#pragma unroll 1
        for (int it = 0; it < per; ++it) {
            const int j = half * per + it;
            const bool mine = floods && j < j_end;
            const int s0 = mine ? st.head[j] : 0, s1 = mine ? st.head[j + 1] : 0;
            const int env = mine ? st.env[s0] : -1;
            uint32_t src = 0;
            if (env >= 0) {
                if (env != cur_env) {                                       // the previous head's world stays in `fr`
                    uint32_t goals, open = 0;
                    if (r < H) open = nav_open_row(type, state, (size_t)env * HW + (size_t)r * W, W, pass_types, doors_open, goals);
#pragma unroll
                    for (int p = 0; p < P; ++p) fr[p] = r < H ? open & ~blocked[(int64_t)env * bstride + p * H + r] : 0u;
                    cur_env = env;
                }
                const int gc = st.goal[s0], gy = gc / W;
                if (r == gy) src = 1u << (gc - gy * W);
                nav_image_clear(img, r, P * cells / 8);                     // every state starts unreachable
            }
            nav_wave_sync();                                                // before other lanes write rounds into it
            nav_timed_seed<P>(img, cells, r, W, src, fr, reached);          // src = 0: nothing is reached, nothing written
            nav_timed_flood<P>(img, cells, r, W, HW * P, fr, reached);
            nav_wave_sync();
            for (int i = s0 + r; i < s1; i += 32) label(i, img, env >= 0);
            nav_wave_sync();                                                // the labels are read before the image is reset
        }
    }
}

// mg_nav_timed_goal_kernel keeps the two spans of its outputs as it had them before nav_out_span_t served every kernel:
// on nav_out_span / nav_out_store it measured 0.9 % slower.  At P = 6 that form has 2034 instructions
// for 2029: 3 v_cmp_lt_i64, 4 s_cselect_b32, 2 v_mov_b64 more, 3 v_writelane and 5 v_readlane fewer; same registers.
struct nav_goal_share_t {
    int sm, sd;
    mg_row_span_t<int64_t> km, kd;
    int64_t bm, bd;                                     // record of LDS slot 0 of either image
    int64_t p0;                                         // record of slot 0 of the key arrays
    bool has_m, has_d;
    int slot_lo, slot_hi;                               // 0 < slot_lo <= slot_hi <= SLOTS, or both 0: no record
};

__device__ __forceinline__ nav_goal_share_t nav_goal_share(const uint8_t *moves, const uint16_t *acting_dist, int64_t M,
                                                           int64_t b)
{
    nav_goal_share_t g;
    g.sm = mg_row_misalign(moves, 16);
    g.sd = acting_dist ? mg_row_misalign(acting_dist, 8) : 0;
    g.km = mg_row_span<int64_t>(g.sm, M, b, NAV_GOAL_ELEMS / 16, 16);
    g.kd = mg_row_span<int64_t>(g.sd, M, b, NAV_GOAL_ELEMS / 8, 8);
    g.bm = 16 * g.km.c0 - g.sm;
    g.bd = 8 * g.kd.c0 - g.sd;
    g.has_m = g.km.c0 < g.km.c1;
    g.has_d = acting_dist != nullptr && g.kd.c0 < g.kd.c1;
    g.p0 = (int64_t)NAV_GOAL_ELEMS * b - 16;
    int64_t lo = 0, hi = 0;                                                 // the records of this workgroup: both spans
    if (g.has_m) { lo = g.km.p_lo; hi = g.km.p_hi; }
    if (g.has_d) { lo = g.has_m && lo < g.kd.p_lo ? lo : g.kd.p_lo; hi = g.has_m && hi > g.kd.p_hi ? hi : g.kd.p_hi; }
    // a workgroup that holds neither span (the last one may) has no slots
    g.slot_lo = g.has_m || g.has_d ? (int)(lo - g.p0) : 0;
    g.slot_hi = g.has_m || g.has_d ? (int)(hi - g.p0) : 0;
    return g;
}

// the label of the record in slot i, parked for the stores
__device__ __forceinline__ void nav_goal_label(nav_goal_stage_t &st, const nav_goal_share_t &g, int i, uint32_t m, uint32_t d)
{
    const int64_t p = g.p0 + i;
    if (g.has_m && p >= g.km.p_lo && p < g.km.p_hi) st.moves[(int)(p - g.bm)] = (uint8_t)m;
    if (g.has_d && p >= g.kd.p_lo && p < g.kd.p_hi) st.dist[(int)(p - g.bd)] = (uint16_t)d;
}

// both outputs leave through the aligned row store; after a __syncthreads()
__device__ __forceinline__ void nav_goal_store(const nav_goal_stage_t &st, const nav_goal_share_t &g, int64_t M,
                                               uint8_t *__restrict__ moves, uint16_t *__restrict__ acting_dist)
{
    const int tid = threadIdx.x;
    for (int64_t c = g.km.c0 + tid; c < g.km.c1; c += NAV_GOAL_THREADS)
        mg_row_store(moves, M, c, [&](int64_t p) { return *reinterpret_cast<const uint4 *>(st.moves + (int)(p - g.bm)); },
                     [&](int64_t q) { return st.moves[(int)(q - g.bm)]; });
    if (acting_dist != nullptr)
        for (int64_t c = g.kd.c0 + tid; c < g.kd.c1; c += NAV_GOAL_THREADS)
            mg_row_store(acting_dist, M, c,
                         [&](int64_t p) { return *reinterpret_cast<const uint4 *>(st.dist + (int)(p - g.bd)); },
                         [&](int64_t q) { return st.dist[(int)(q - g.bd)]; });
}

template <int P> __global__ __launch_bounds__(NAV_GOAL_THREADS) void mg_nav_timed_goal_kernel(
    const uint8_t *__restrict__ type, const uint8_t *__restrict__ state, int N, int W, int H, uint32_t pass_types,
    int doors_open, const uint32_t *__restrict__ blocked, int64_t bstride, const int32_t *__restrict__ rec_t,
    const int32_t *__restrict__ rec_n, const float *__restrict__ rec_goal, int64_t M, const float2 *__restrict__ pos,
    const int32_t *__restrict__ age, const float *__restrict__ init_pos, int T, uint8_t *__restrict__ moves,
    uint16_t *__restrict__ acting_dist, int flooders)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t goal_image[];   // [flooders][P][cells]
    __shared__ nav_goal_stage_t st;
    __shared__ uint8_t s_phase[NAV_GOAL_SLOTS];                             // the phase of a record's clock
    const nav_goal_share_t g = nav_goal_share(moves, acting_dist, M, blockIdx.x);
    const int cells = nav_timed_cells(W * H);

    nav_goal_keys<true>(st, s_phase, g, N, W, H, P, rec_t, rec_n, rec_goal, pos, age, init_pos, T, nav_goal_no_more);
    const int n_heads = nav_goal_heads(st, g);
    nav_timed_goal_floods<P>(st, goal_image, n_heads, flooders, type, state, W, H, pass_types, doors_open, blocked, bstride,
                             [&](int i, const uint16_t *img, bool ok) {
                                 const int c = st.cell[i], ph = s_phase[i];
                                 uint32_t d = MG_NAV_UNREACHABLE, m = 0;
                                 if (ok && c != NAV_NO_CELL)
                                     m = nav_move_set<true>(img + ph * cells, img + (ph + 1 == P ? 0 : ph + 1) * cells, c, W,
                                                            H, d);
                                 nav_goal_label(st, g, i, m, d);
                             });
    __syncthreads();
    nav_goal_store(st, g, M, moves, acting_dist);
}

// ------------------------------------------------------------------ potential-based reward shaping from the fields
// The three float operations of minigrid_nav.h ("Reward shaping"), each rounded once: nothing here may fuse.
__device__ __forceinline__ float nav_phi(float scale, uint32_t d)
{
#pragma clang fp contract(off)
    if (d == 0u) return 0.0f;
    const float m = scale * (float)d;
    return -m;
}
__device__ __forceinline__ float nav_shaping(float gamma, float phi_after, float phi_before)
{
#pragma clang fp contract(off)
    const float g = gamma * phi_after;
    return g - phi_before;
}
__device__ __forceinline__ float nav_shaped(float reward, float F)
{
#pragma clang fp contract(off)
    return reward + F;
}

// F of a pair of distances and whether the element is shaped at all; terminal: phi_after = 0 whatever d_after is.
__device__ __forceinline__ bool nav_shape_term(uint32_t d_before, uint32_t d_after, bool terminal, float scale, float gamma,
                                               float &F)
{
    F = 0.0f;
    if (d_before == (uint32_t)MG_NAV_UNREACHABLE || (!terminal && d_after == (uint32_t)MG_NAV_UNREACHABLE)) return false;
    F = nav_shaping(gamma, terminal ? 0.0f : nav_phi(scale, d_after), nav_phi(scale, d_before));
    return true;
}

static_assert(NAV_MOVES_ELEMS % 16 == 0 && NAV_MOVES_ELEMS % 4 == 0, "whole chunks of the float outputs and of the mask");

// TIMED: dist holds P fields per env and the phases come from the element's age; done is given iff the terminal rule is on.
template <bool TIMED> __global__ __launch_bounds__(NAV_MOVES_THREADS) void mg_nav_shape_kernel(
    const uint16_t *__restrict__ dist, int64_t pitch, int P, int N, int W, int H, const float2 *__restrict__ pos_before,
    const float2 *__restrict__ pos_after, const int32_t *__restrict__ age, const float *__restrict__ init_pos,
    const uint8_t *__restrict__ done, const float *reward, int64_t M, float scale, float gamma, float *reward_out,
    float *__restrict__ shaping, uint8_t *__restrict__ mask)
{
    __shared__ __attribute__((aligned(16))) float s_out[NAV_MOVES_ELEMS];
    __shared__ __attribute__((aligned(16))) float s_f[NAV_MOVES_ELEMS];
    __shared__ __attribute__((aligned(16))) uint8_t s_mask[NAV_MOVES_ELEMS];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    // this workgroup's chunks of each output and the elements they hold: all within [ELEMS * b - 15, ELEMS * (b + 1))
    const nav_out_span_t so = nav_out_span(reward_out, M, b, NAV_MOVES_ELEMS);
    const nav_out_span_t sf = nav_out_span(shaping, M, b, NAV_MOVES_ELEMS);
    const nav_out_span_t sm = nav_out_span(mask, M, b, NAV_MOVES_ELEMS);
    const int HW = W * H;
    float2 init = make_float2(0.f, 0.f);
    if (age != nullptr) init = make_float2(init_pos[0], init_pos[1]);

    const int64_t p0 = (int64_t)NAV_MOVES_ELEMS * b - 16;
#pragma unroll 1
    for (int k = 0; k < NAV_MOVES_ROUNDS; ++k) {
        const int64_t p = p0 + k * NAV_MOVES_THREADS + tid;
        const bool in_o = so.holds(p), in_f = sf.holds(p), in_m = sm.holds(p);
        if (!(in_o || in_f || in_m)) continue;                              // every span lies inside [0, M)
        float2 q = pos_before[p];
        const float2 qa = pos_after[p];
        const int clock = age != nullptr ? age[p] : 1;
        if (clock <= 0) q = init;
        const int cb = visit_cell(q.x, q.y, W, H), ca = visit_cell(qa.x, qa.y, W, H);
        const bool terminal = done != nullptr && done[p] != 0;
        const uint16_t *fb = dist + (int64_t)(p % N) * P * pitch, *fa = fb;
        if (TIMED) {                                                        // the after state's clock is max(clock, 0) + 1
            const int ph = nav_phase(clock, P);
            fb += ph * pitch;
            fa += (ph + 1 >= P ? 0 : ph + 1) * pitch;
        }
        const uint32_t db = cb < HW ? fb[cb] : (uint32_t)MG_NAV_UNREACHABLE;
        const uint32_t da = ca < HW && !terminal ? fa[ca] : (uint32_t)MG_NAV_UNREACHABLE;
        float F;
        const bool shaped = nav_shape_term(db, da, terminal, scale, gamma, F);
        if (in_o) {                                                         // read before the barrier, by the workgroup that
            const float r = reward[p];                                      // stores it: reward_out may be reward itself
            s_out[(int)(p - so.base)] = shaped ? nav_shaped(r, F) : r;
        }
        if (in_f) s_f[(int)(p - sf.base)] = F;
        if (in_m) s_mask[(int)(p - sm.base)] = shaped ? 1 : 0;
    }
    __syncthreads();
    nav_out_store(reward_out, M, so, s_out, NAV_MOVES_THREADS);
    nav_out_store(shaping, M, sf, s_f, NAV_MOVES_THREADS);
    nav_out_store(mask, M, sm, s_mask, NAV_MOVES_THREADS);
}

// What the goal kernel's staging lacks for shaping: the after-step cell of a record and the three outputs on their way out.
constexpr uint16_t NAV_TERMINAL = 0xFFFE;               // an after-step "cell": the terminal rule applies, phi_after = 0
struct nav_goal_shape_stage_t {
    alignas(16) float out[NAV_GOAL_ELEMS];              // the record's reward from the keys on, shaped by its label
    alignas(16) float f[NAV_GOAL_ELEMS];
    alignas(16) uint8_t mask[NAV_GOAL_ELEMS];
    uint16_t after[NAV_GOAL_SLOTS];                     // NAV_NO_CELL where the position is none, NAV_TERMINAL
};
static_assert(NAV_CELLS < NAV_TERMINAL, "the two marks are no cells");
static_assert(sizeof(nav_goal_stage_t) + sizeof(nav_goal_shape_stage_t) + NAV_GOAL_HALVES * NAV_CELLS * sizeof(uint16_t) + 64
                  <= 64 * 1024, "the staging of a shaping workgroup fits 64 KiB next to its 8 images");

// What a shaping kernel keeps of record p (slot i, element `at` or -1) besides its keys: nav_goal_keys' `more`.
__device__ __forceinline__ void nav_goal_shape_more(nav_goal_shape_stage_t &sh, const nav_out_span_t &so, int i, int64_t p,
                                                    int64_t at, const uint8_t *__restrict__ rec_done,
                                                    const float *rec_reward, const float2 *__restrict__ pos_after, int W,
                                                    int H)
{
    int a = NAV_NO_CELL;
    if (at >= 0) {
        if (rec_done != nullptr && rec_done[p] != 0) a = NAV_TERMINAL;
        else {
            const float2 q = pos_after[at];
            const int c = visit_cell(q.x, q.y, W, H);
            if (c < W * H) a = c;
        }
    }
    sh.after[i] = (uint16_t)a;
    // read before the barrier, by the workgroup that stores it: reward_out may be rec_reward
    if (so.holds(p)) sh.out[(int)(p - so.base)] = rec_reward[p];
}

// The shaping label of record p in slot i, parked for the stores: its acting cell c is read in `before`, its after cell
// in `after` (one image for a static field, the acting and the following phase's for a timed one); ok = the run has a result.
__device__ __forceinline__ void nav_goal_shape_label(nav_goal_shape_stage_t &sh, const nav_out_span_t &so,
                                                     const nav_out_span_t &sf, const nav_out_span_t &sm, int64_t p, int i,
                                                     int c, const uint16_t *before, const uint16_t *after, bool ok,
                                                     float scale, float gamma)
{
    const int a = sh.after[i];
    float F = 0.0f;
    bool shaped = false;
    if (ok && c != NAV_NO_CELL && a != NAV_NO_CELL)
        shaped = nav_shape_term(before[c], a == NAV_TERMINAL ? (uint32_t)MG_NAV_UNREACHABLE : after[a], a == NAV_TERMINAL,
                                scale, gamma, F);
    if (shaped && so.holds(p)) {
        float &o = sh.out[(int)(p - so.base)];
        o = nav_shaped(o, F);
    }
    if (sf.holds(p)) sh.f[(int)(p - sf.base)] = F;
    if (sm.holds(p)) sh.mask[(int)(p - sm.base)] = shaped ? 1 : 0;
}

__global__ __launch_bounds__(NAV_GOAL_THREADS) void mg_nav_goal_shape_kernel(
    const uint8_t *__restrict__ type, const uint8_t *__restrict__ state, int N, int W, int H, uint32_t pass_types,
    int doors_open, const int32_t *__restrict__ rec_t, const int32_t *__restrict__ rec_n,
    const float *__restrict__ rec_goal, const uint8_t *__restrict__ rec_done, const float *rec_reward, int64_t M,
    const float2 *__restrict__ pos_before, const float2 *__restrict__ pos_after, const int32_t *__restrict__ age,
    const float *__restrict__ init_pos, int T, float scale, float gamma, float *reward_out, float *__restrict__ shaping,
    uint8_t *__restrict__ mask)
{
    __shared__ __attribute__((aligned(16))) uint16_t image[NAV_GOAL_HALVES][NAV_CELLS];
    __shared__ nav_goal_stage_t st;
    __shared__ nav_goal_shape_stage_t sh;
    const nav_out_span_t so = nav_out_span(reward_out, M, blockIdx.x, NAV_GOAL_ELEMS);
    const nav_out_span_t sf = nav_out_span(shaping, M, blockIdx.x, NAV_GOAL_ELEMS);
    const nav_out_span_t sm = nav_out_span(mask, M, blockIdx.x, NAV_GOAL_ELEMS);
    const nav_goal_records_t g = nav_goal_records(M, blockIdx.x, so, sf, sm);

    nav_goal_keys<false>(st, nullptr, g, N, W, H, 1, rec_t, rec_n, rec_goal, pos_before, age, init_pos, T,
                         [&](int i, int64_t p, int64_t at) {
                             nav_goal_shape_more(sh, so, i, p, at, rec_done, rec_reward, pos_after, W, H);
                         });
    const int n_heads = nav_goal_heads(st, g);
    nav_goal_floods(st, image[threadIdx.x >> 5], n_heads, type, state, W, H, pass_types, doors_open,
                    [&](int i, const uint16_t *img, bool ok) {
                        nav_goal_shape_label(sh, so, sf, sm, g.p0 + i, i, st.cell[i], img, img, ok, scale, gamma);
                    });
    __syncthreads();
    nav_out_store(reward_out, M, so, sh.out, NAV_GOAL_THREADS);
    nav_out_store(shaping, M, sf, sh.f, NAV_GOAL_THREADS);
    nav_out_store(mask, M, sm, sh.mask, NAV_GOAL_THREADS);
}

// ------------------------------------------------------------------ timed shaping of records with goals of their own
// mg_nav_goal_shape_kernel over (cell, phase): the timed goal kernel's keys, heads and floods (nav_timed_goal_floods), the
// goal shaping kernel's after cells, label and stores.  The label reads two phase images: the acting phase's for the acting
// cell, the following phase's for the after cell.  Its staging is larger than the move sets', so it has a host choice of
// its own: MG_NAV_TIMED_GOAL_SHAPE_LDS is what the images share 64 KiB with (static LDS and what aligning it may cost).
static_assert(sizeof(nav_goal_stage_t) + NAV_GOAL_SLOTS + sizeof(nav_goal_shape_stage_t) + 64 == MG_NAV_TIMED_GOAL_SHAPE_LDS,
              "the header states the byte count of the formula");
static_assert(MG_NAV_TIMED_GOAL_SHAPE_LDS + NAV_MAX_PERIOD * NAV_CELLS * sizeof(uint16_t) <= 64 * 1024,
              "one image of the longest period and the largest world fits next to the shaping staging");

template <int P> __global__ __launch_bounds__(NAV_GOAL_THREADS) void mg_nav_timed_goal_shape_kernel(
    const uint8_t *__restrict__ type, const uint8_t *__restrict__ state, int N, int W, int H, uint32_t pass_types,
    int doors_open, const uint32_t *__restrict__ blocked, int64_t bstride, const int32_t *__restrict__ rec_t,
    const int32_t *__restrict__ rec_n, const float *__restrict__ rec_goal, const uint8_t *__restrict__ rec_done,
    const float *rec_reward, int64_t M, const float2 *__restrict__ pos_before, const float2 *__restrict__ pos_after,
    const int32_t *__restrict__ age, const float *__restrict__ init_pos, int T, float scale, float gamma, float *reward_out,
    float *__restrict__ shaping, uint8_t *__restrict__ mask, int flooders)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t goal_shape_image[];   // [flooders][P][cells]
    __shared__ nav_goal_stage_t st;
    __shared__ nav_goal_shape_stage_t sh;
    __shared__ uint8_t s_phase[NAV_GOAL_SLOTS];                             // the phase of a record's clock
    const int HW = W * H, cells = nav_timed_cells(HW);
    const nav_out_span_t so = nav_out_span(reward_out, M, blockIdx.x, NAV_GOAL_ELEMS);
    const nav_out_span_t sf = nav_out_span(shaping, M, blockIdx.x, NAV_GOAL_ELEMS);
    const nav_out_span_t sm = nav_out_span(mask, M, blockIdx.x, NAV_GOAL_ELEMS);
    const nav_goal_records_t g = nav_goal_records(M, blockIdx.x, so, sf, sm);

    nav_goal_keys<true>(st, s_phase, g, N, W, H, P, rec_t, rec_n, rec_goal, pos_before, age, init_pos, T,
                        [&](int i, int64_t p, int64_t at) {
                            nav_goal_shape_more(sh, so, i, p, at, rec_done, rec_reward, pos_after, W, H);
                        });
    const int n_heads = nav_goal_heads(st, g);
    nav_timed_goal_floods<P>(st, goal_shape_image, n_heads, flooders, type, state, W, H, pass_types, doors_open, blocked,
                             bstride, [&](int i, const uint16_t *img, bool ok) {
                                 const int ph = s_phase[i];                 // the after state's phase follows the acting one
                                 nav_goal_shape_label(sh, so, sf, sm, g.p0 + i, i, st.cell[i], img + ph * cells,
                                                      img + (ph + 1 == P ? 0 : ph + 1) * cells, ok, scale, gamma);
                             });
    __syncthreads();
    nav_out_store(reward_out, M, so, sh.out, NAV_GOAL_THREADS);
    nav_out_store(shaping, M, sf, sh.f, NAV_GOAL_THREADS);
    nav_out_store(mask, M, sm, sh.mask, NAV_GOAL_THREADS);
}

// ------------------------------------------------------------------ timed look-ahead labels of records with goals of their own
// mg_nav_goal_ahead_kernel over (cell, phase): the timed goal kernel's keys, heads and floods (nav_timed_goal_floods), the
// look-ahead kernel's label, staging and stores.  The label walks the half wavefront's P images, `cells` apart, from the
// record's phase on.  Its staging is the move sets' plus the 8 KiB of labels, so it has a host choice of its own:
// MG_NAV_TIMED_GOAL_AHEAD_LDS is what the images share 64 KiB with (static LDS and what aligning it may cost).
static_assert(sizeof(nav_goal_stage_t) + NAV_GOAL_SLOTS + sizeof(nav_goal_ahead_stage_t) + 64 == MG_NAV_TIMED_GOAL_AHEAD_LDS,
              "the header states the byte count of the formula");
static_assert(MG_NAV_TIMED_GOAL_AHEAD_LDS + NAV_MAX_PERIOD * NAV_CELLS * sizeof(uint16_t) <= 64 * 1024,
              "one image of the longest period and the largest world fits next to the look-ahead staging");

template <int P> __global__ __launch_bounds__(NAV_GOAL_THREADS) void mg_nav_timed_goal_ahead_kernel(
    const uint8_t *__restrict__ type, const uint8_t *__restrict__ state, int N, int W, int H, uint32_t pass_types,
    int doors_open, const uint32_t *__restrict__ blocked, int64_t bstride, const int32_t *__restrict__ rec_t,
    const int32_t *__restrict__ rec_n, const float *__restrict__ rec_goal, int64_t M, const float2 *__restrict__ pos,
    const int32_t *__restrict__ age, const float *__restrict__ init_pos, int T, int steps,
    unsigned long long *__restrict__ ahead, uint16_t *__restrict__ acting_dist, int flooders)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t goal_ahead_image[];   // [flooders][P][cells]
    __shared__ nav_goal_stage_t st;
    __shared__ nav_goal_ahead_stage_t sh;
    __shared__ uint8_t s_phase[NAV_GOAL_SLOTS];                             // the phase of a record's clock
    const int cells = nav_timed_cells(W * H);
    const nav_out_span_t sa = nav_out_span(ahead, M, blockIdx.x, NAV_GOAL_ELEMS);
    const nav_out_span_t sd = nav_out_span(acting_dist, M, blockIdx.x, NAV_GOAL_ELEMS);
    const nav_goal_records_t g = nav_goal_records(M, blockIdx.x, sa, sd);

    nav_goal_keys<true>(st, s_phase, g, N, W, H, P, rec_t, rec_n, rec_goal, pos, age, init_pos, T, nav_goal_no_more);
    const int n_heads = nav_goal_heads(st, g);
    nav_timed_goal_floods<P>(st, goal_ahead_image, n_heads, flooders, type, state, W, H, pass_types, doors_open, blocked,
                             bstride, [&](int i, const uint16_t *img, bool ok) {
                                 const int c = st.cell[i], ph = s_phase[i];
                                 const int64_t p = g.p0 + i;
                                 uint32_t d = MG_NAV_UNREACHABLE;
                                 uint64_t a = 0;
                                 if (ok && c != NAV_NO_CELL) a = nav_ahead_label<true>(img, cells, P, ph, c, W, H, steps, d);
                                 if (sa.holds(p)) sh.ahead[(int)(p - sa.base)] = a;
                                 if (sd.holds(p)) st.dist[(int)(p - sd.base)] = (uint16_t)d;
                             });
    __syncthreads();
    nav_out_store(ahead, M, sa, sh.ahead, NAV_GOAL_THREADS);
    nav_out_store(acting_dist, M, sd, st.dist, NAV_GOAL_THREADS);
}

// ------------------------------------------------------------------ path efficiency per episode
// The scan of minigrid_nav.h ("Path efficiency"): ppo_episode_scan's shape, a lane per env over coalesced rows [t][n].  The
// dependent chain is four integer operations per step; what costs is the two gathers per step from the env's field, so the
// loads and gathers of NAV_PATH_ROWS rows are issued together, ahead of the chain (rows past T repeat row T - 1 and are
// dropped: every load of a batch is unconditional).  TIMED: dist holds P fields per env, the phases come from the age.
constexpr int NAV_PATH_THREADS = 64, NAV_PATH_ROWS = 8;

template <bool TIMED> __global__ __launch_bounds__(NAV_PATH_THREADS) void mg_nav_path_scan_kernel(
    const uint16_t *__restrict__ dist, int64_t pitch, int P, int N, int W, int H, const float2 *__restrict__ pos_before,
    const float2 *__restrict__ pos_after, const int32_t *__restrict__ age, const float *__restrict__ init_pos,
    const uint8_t *__restrict__ terminated, const uint8_t *__restrict__ truncated, int T,
    uint16_t *__restrict__ carry_start, uint16_t *__restrict__ carry_best, int32_t *__restrict__ carry_off,
    int32_t *__restrict__ carry_steps, uint16_t *__restrict__ ep_start, uint16_t *__restrict__ ep_best,
    int32_t *__restrict__ ep_off, int32_t *__restrict__ ep_steps)
{
    const int n = blockIdx.x * NAV_PATH_THREADS + threadIdx.x;
    if (n >= N) return;
    const int HW = W * H;
    const uint16_t *f = dist + (int64_t)n * P * pitch;
    float2 init = make_float2(0.f, 0.f);
    if (age != nullptr) init = make_float2(init_pos[0], init_pos[1]);
    uint32_t start = carry_start[n], best = carry_best[n];
    int off = carry_off[n], steps = carry_steps[n];
    for (int t0 = 0; t0 < T; t0 += NAV_PATH_ROWS) {
        uint32_t db[NAV_PATH_ROWS], da[NAV_PATH_ROWS], dn[NAV_PATH_ROWS];
#pragma unroll
        for (int j = 0; j < NAV_PATH_ROWS; ++j) {
            const int t = t0 + j < T ? t0 + j : T - 1;
            const int64_t i = (int64_t)t * N + n;
            float2 q = pos_before[i];
            const float2 qa = pos_after[i];
            const int clock = age != nullptr ? age[i] : 1;
            if (clock <= 0) q = init;
            const int cb = visit_cell(q.x, q.y, W, H), ca = visit_cell(qa.x, qa.y, W, H);
            const uint16_t *fb = f, *fa = f;
            if (TIMED) {                                                    // as mg_nav_shape_kernel takes its two rows
                const int ph = nav_phase(clock, P);
                fb += ph * pitch;
                fa += (ph + 1 >= P ? 0 : ph + 1) * pitch;
            }
            db[j] = cb < HW ? fb[cb] : (uint32_t)MG_NAV_UNREACHABLE;
            da[j] = ca < HW ? fa[ca] : (uint32_t)MG_NAV_UNREACHABLE;
            dn[j] = (uint32_t)(terminated[i] | truncated[i]);
        }
#pragma unroll
        for (int j = 0; j < NAV_PATH_ROWS; ++j) {
            const int t = t0 + j;
            if (t < T) {
                const int64_t i = (int64_t)t * N + n;
                if (steps == 0) { start = best = db[j]; off = 0; }
                steps += 1;
                const bool on_path = db[j] != (uint32_t)MG_NAV_UNREACHABLE && db[j] >= 1u && da[j] == db[j] - 1u;
                off += on_path ? 0 : 1;
                best = da[j] < best ? da[j] : best;
                if (ep_start) ep_start[i] = (uint16_t)start;
                if (ep_best) ep_best[i] = (uint16_t)best;
                if (ep_off) ep_off[i] = off;
                if (ep_steps) ep_steps[i] = steps;
                if (dn[j]) steps = 0;
            }
        }
    }
    carry_start[n] = (uint16_t)start;
    carry_best[n] = (uint16_t)best;
    carry_off[n] = off;
    carry_steps[n] = steps;
}

// The summary of minigrid_nav.h: ppo_episode_summary's two kernels and its order of combination (ppo_kernels.hip) on a
// partial of NAV_PATH_NV doubles -- every entry a sum but the last, a minimum.  Counts and integer sums are kept as integers
// per thread and are exact as doubles from there on (far below 2^53).
constexpr int NAV_PATH_NV = MG_NAV_PATH_SUMMARY, NAV_PATH_MIN = NAV_PATH_NV - 1;
constexpr int NAV_PATH_BLOCK_ELEMS = 2048, NAV_PATH_MAX_BLOCKS = 256, NAV_PATH_SUM_THREADS = 256;

__device__ __forceinline__ void nav_path_combine(double (&v)[NAV_PATH_NV], const double (&w)[NAV_PATH_NV])
{
#pragma unroll
    for (int k = 0; k < NAV_PATH_MIN; ++k) v[k] += w[k];
    v[NAV_PATH_MIN] = fmin(v[NAV_PATH_MIN], w[NAV_PATH_MIN]);
}

// Ordered over the 64 lanes: after step s a lane whose index is a multiple of 2s holds lanes [lane, lane + 2s) in lane order.
__device__ __forceinline__ void nav_path_wave_reduce(double (&v)[NAV_PATH_NV])
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        double w[NAV_PATH_NV];
#pragma unroll
        for (int k = 0; k < NAV_PATH_NV; ++k) w[k] = __shfl_down(v[k], s, 64);
        nav_path_combine(v, w);
    }
}

__global__ __launch_bounds__(NAV_PATH_SUM_THREADS) void mg_nav_path_partial_kernel(
    const uint16_t *__restrict__ ep_start, const uint16_t *__restrict__ ep_best, const int32_t *__restrict__ ep_off,
    const int32_t *__restrict__ ep_steps, const uint8_t *__restrict__ terminated, const uint8_t *__restrict__ truncated,
    int64_t M, int64_t per_block, int per_thread, double *__restrict__ ws)
{
    __shared__ double sh[NAV_PATH_SUM_THREADS / 64][NAV_PATH_NV];
    const int64_t block_lo = (int64_t)blockIdx.x * per_block;
    const int64_t block_hi = block_lo + per_block < M ? block_lo + per_block : M;
    const int64_t lo = block_lo + (int64_t)threadIdx.x * per_thread;
    const int64_t hi = lo + per_thread < block_hi ? lo + per_thread : block_hi;
    long long episodes = 0, successes = 0, rated = 0, sum_start = 0, sum_best = 0, sum_off = 0, sum_steps = 0;
    uint32_t min_best = MG_NAV_UNREACHABLE;                                 // of the rated: reachable, so below this
    double spl = 0.0, progress = 0.0;
    for (int64_t i = lo; i < hi; ++i) {
        const uint32_t te = terminated[i];
        if (!(te | truncated[i])) continue;                                 // an episode ends here
        const uint32_t s = ep_start[i], b = ep_best[i];
        const int st = ep_steps[i];
        episodes += 1;
        successes += te ? 1 : 0;
        sum_off += ep_off[i];
        sum_steps += st;
        if (s == (uint32_t)MG_NAV_UNREACHABLE) continue;
        rated += 1;
        sum_start += s;
        sum_best += b;
        min_best = b < min_best ? b : min_best;
        if (te) spl += (double)s / (double)(st > (int)s ? st : (int)s);
        if (s >= 1u) progress += (double)((int)s - (int)b) / (double)s;      // the scan keeps best <= start
    }
    double v[NAV_PATH_NV] = {(double)episodes, (double)successes, (double)rated, spl, (double)sum_start, (double)sum_best,
                             progress, (double)sum_off, (double)sum_steps,
                             rated ? (double)min_best : (double)INFINITY};
    nav_path_wave_reduce(v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NAV_PATH_NV; ++k) sh[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NAV_PATH_SUM_THREADS / 64; ++w) {               // wavefronts in index order
            double o[NAV_PATH_NV];
#pragma unroll
            for (int k = 0; k < NAV_PATH_NV; ++k) o[k] = sh[w][k];
            nav_path_combine(v, o);
        }
#pragma unroll
        for (int k = 0; k < NAV_PATH_NV; ++k) ws[(size_t)blockIdx.x * NAV_PATH_NV + k] = v[k];
    }
}

__global__ __launch_bounds__(64) void mg_nav_path_finalize_kernel(const double *__restrict__ ws, int nblocks,
                                                                  double *__restrict__ summary)
{
    const int lane = threadIdx.x;
    const int per_lane = (nblocks + 63) / 64;                               // nblocks <= NAV_PATH_MAX_BLOCKS: at most 4 each
    double v[NAV_PATH_NV] = {};
    v[NAV_PATH_MIN] = (double)INFINITY;
    for (int j = 0; j < per_lane; ++j) {                                    // lane l: blocks [l * per_lane, (l + 1) * per_lane)
        const int blk = lane * per_lane + j;
        if (blk < nblocks) {
            double o[NAV_PATH_NV];
#pragma unroll
            for (int k = 0; k < NAV_PATH_NV; ++k) o[k] = ws[(size_t)blk * NAV_PATH_NV + k];
            nav_path_combine(v, o);
        }
    }
    nav_path_wave_reduce(v);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NAV_PATH_NV; ++k) summary[k] = v[k];
    }
}

// ------------------------------------------------------------------ the argument rules of minigrid_nav.h, each once
bool nav_sides_ok(int W, int H) { return W >= 1 && W <= NAV_SIDE && H >= 1 && H <= NAV_SIDE; }
bool nav_period_ok(int P) { return P >= 1 && P <= NAV_MAX_PERIOD; }
bool nav_flags_ok(int flags, int allowed) { return (flags & ~allowed) == 0; }
bool nav_aligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }       // NULL is aligned
bool nav_count_ok(int64_t count) { return count >= 0 && count < ((int64_t)1 << 40); }     // elements or records of a launch

bool nav_world_ok(const uint8_t *type, int n_envs, int W, int H, uint32_t pass_types, int flags, int allowed)
{
    return type && n_envs > 0 && nav_sides_ok(W, H) && pass_types <= 0xFFFFu && nav_flags_ok(flags, allowed);
}

// fields in memory: rows of W * H distances, dist_pitch elements apart (0: dense); required: dist is no option
bool nav_field_ok(const uint16_t *dist, int64_t dist_pitch, int n_envs, int W, int H, bool required)
{
    return (dist || !required) && nav_aligned(dist, 2) && n_envs > 0 && nav_sides_ok(W, H) &&
           (dist_pitch == 0 || dist_pitch >= (int64_t)W * H);
}
int64_t nav_pitch(int64_t dist_pitch, int W, int H) { return dist_pitch ? dist_pitch : (int64_t)W * H; }

// the schedule: period * height words per env, blocked_env_stride words apart (0: one schedule for all envs)
bool nav_schedule_ok(const uint32_t *blocked, int64_t blocked_env_stride, int period, int height)
{
    return nav_period_ok(period) && blocked && nav_aligned(blocked, 4) &&
           (blocked_env_stride == 0 || blocked_env_stride >= (int64_t)period * height);
}

// goals and agents: x and y come together, each pair with a positive stride; wanted: an output or the clock asks for the agent
bool nav_agents_ok(const int32_t *goal_x, const int32_t *goal_y, int goal_stride, const int32_t *agent_x,
                   const int32_t *agent_y, int agent_stride, bool wanted)
{
    return (goal_x == nullptr) == (goal_y == nullptr) && (agent_x == nullptr) == (agent_y == nullptr) &&
           (agent_x || !wanted) && (!goal_x || goal_stride > 0) && (!agent_x || agent_stride > 0);
}

bool nav_records_ok(const int32_t *rec_t, const int32_t *rec_n, const float *rec_goal, int64_t n_records)
{
    return rec_t && rec_n && rec_goal && nav_aligned(rec_t, 4) && nav_aligned(rec_n, 4) && nav_aligned(rec_goal, 4) &&
           nav_count_ok(n_records);
}

bool nav_rollout_ok(const float *pos, int T) { return pos && nav_aligned(pos, 8) && T >= 0; }

// the clock: age comes with init_pos; required: the age is the clock of a timed field, both must be given
bool nav_clock_ok(const int32_t *age, const float *init_pos, bool required)
{
    return (required ? age && init_pos : !age || init_pos) && nav_aligned(age, 4) && nav_aligned(init_pos, 4);
}

// A record launch: the world (flags against the mask the entry point admits), the schedule where the launch is timed, the
// records, the rollout's position arrays (pos_after = pos where there is one) and the clock -- required where timed.
bool nav_record_launch_ok(const uint8_t *type, int n_envs, int W, int H, uint32_t pass_types, int flags, int allowed, bool timed,
                          const uint32_t *blocked, int64_t blocked_env_stride, int period, const int32_t *rec_t,
                          const int32_t *rec_n, const float *rec_goal, int64_t n_records, const float *pos,
                          const float *pos_after, const int32_t *age, const float *init_pos, int T)
{
    return nav_world_ok(type, n_envs, W, H, pass_types, flags, allowed) &&
           (!timed || nav_schedule_ok(blocked, blocked_env_stride, period, H)) &&
           nav_records_ok(rec_t, rec_n, rec_goal, n_records) && nav_rollout_ok(pos, T) && nav_rollout_ok(pos_after, T) &&
           nav_clock_ok(age, init_pos, timed);
}
// A rollout launch on fields of a period: the fields, the period, the position arrays (pos_after = pos where there is one),
// the clock and the element count.
bool nav_rollout_launch_ok(const uint16_t *dist, int64_t dist_pitch, int period, int n_envs, int W, int H, const float *pos,
                           const float *pos_after, const int32_t *age, const float *init_pos, bool clock_required, int T)
{
    return nav_field_ok(dist, dist_pitch, n_envs, W, H, true) && nav_period_ok(period) && nav_rollout_ok(pos, T) &&
           nav_rollout_ok(pos_after, T) && nav_clock_ok(age, init_pos, clock_required) && nav_count_ok((int64_t)T * n_envs);
}
// the mg_nav_timed_goal*_floods queries: the launch's own count next to its `fixed` bytes
int nav_floods_query(size_t fixed, int W, int H, int period)
{
    return nav_sides_ok(W, H) && nav_period_ok(period) ? nav_timed_goal_flooders(fixed, W * H, period) : TW_E_ARG;
}

bool nav_moves_out_ok(const uint8_t *moves, const uint16_t *acting_dist) { return moves && nav_aligned(acting_dist, 2); }
bool nav_ahead_out_ok(int steps, const uint64_t *ahead, const uint16_t *acting_dist)
{
    return steps >= 1 && steps <= MG_NAV_AHEAD_MAX_STEPS && ahead && nav_aligned(ahead, 8) && nav_aligned(acting_dist, 2);
}
// shaping: an output at least, reward_out with a reward, the terminal flag with done, finite scale and gamma
bool nav_shaping_ok(const float *reward, const uint8_t *done, int flags, float scale, float gamma, const float *reward_out,
                    const float *shaping, const uint8_t *mask)
{
    return (reward_out || shaping || mask) && (!reward_out || reward) && (!(flags & MG_NAV_SHAPE_ZERO_TERMINAL) || done) &&
           nav_aligned(reward, 4) && nav_aligned(reward_out, 4) && nav_aligned(shaping, 4) && __builtin_isfinite(scale) &&
           __builtin_isfinite(gamma);
}
const uint8_t *nav_ends(const uint8_t *done, int flags) { return (flags & MG_NAV_SHAPE_ZERO_TERMINAL) ? done : nullptr; }
// path efficiency: the two flag arrays, and (start, best, off, steps) as carries or as per-step arrays -- required: all four
bool nav_flags_given(const uint8_t *terminated, const uint8_t *truncated) { return terminated && truncated; }
bool nav_path_arrays_ok(const uint16_t *start, const uint16_t *best, const int32_t *off, const int32_t *steps, bool required)
{
    return (required ? start && best && off && steps : start || best || off || steps) && nav_aligned(start, 2) &&
           nav_aligned(best, 2) && nav_aligned(off, 4) && nav_aligned(steps, 4);
}
int nav_path_blocks(int64_t M)
{
    const int64_t b = (M + NAV_PATH_BLOCK_ELEMS - 1) / NAV_PATH_BLOCK_ELEMS;
    return (int)(b < NAV_PATH_MAX_BLOCKS ? b : NAV_PATH_MAX_BLOCKS);
}

// workgroups of `elems` elements: chunks are counted from the aligned address below each output, up to 15 more than count
dim3 nav_grid(int64_t count, int elems) { return dim3((unsigned)((count + 15 + elems - 1) / elems)); }

const float2 *nav_f2(const float *pos) { return reinterpret_cast<const float2 *>(pos); }
}  // namespace

extern "C" int mg_nav_field(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                            uint32_t pass_types, int flags, const int32_t *goal_x, const int32_t *goal_y, int goal_stride,
                            const int32_t *agent_x, const int32_t *agent_y, int agent_stride, uint16_t *dist,
                            int64_t dist_pitch, int32_t *agent_dist, int32_t *agent_action, int32_t *error, void *stream)
{
    if (!nav_world_ok(type, n_envs, width, height, pass_types, flags, MG_NAV_DOORS_OPEN) ||
        !nav_field_ok(dist, dist_pitch, n_envs, width, height, false) ||
        !nav_agents_ok(goal_x, goal_y, goal_stride, agent_x, agent_y, agent_stride, agent_dist || agent_action))
        return TW_E_ARG;
    hipLaunchKernelGGL(mg_nav_field_kernel, dim3((n_envs + NAV_ENVS - 1) / NAV_ENVS), dim3(NAV_THREADS), 0,
                       (hipStream_t)stream, type, state, n_envs, width, height, pass_types, flags & MG_NAV_DOORS_OPEN,
                       goal_x, goal_y, goal_stride, agent_x, agent_y, agent_stride, dist,
                       nav_pitch(dist_pitch, width, height), agent_dist, agent_action, error);
    return tw_launched(__func__);
}

extern "C" int mg_nav_lookup(const uint16_t *dist, int64_t dist_pitch, int n_envs, int width, int height, const float *pos,
                             int T, uint16_t *out, void *stream)
{
    const int64_t M = (int64_t)T * n_envs;
    if (!nav_field_ok(dist, dist_pitch, n_envs, width, height, true) || !nav_rollout_ok(pos, T) || !out ||
        !nav_aligned(out, 2) || !nav_count_ok(M))
        return TW_E_ARG;
    if (M == 0) return TW_OK;
    hipLaunchKernelGGL(mg_nav_lookup_kernel, dim3((unsigned)((M + NAV_LOOKUP_THREADS - 1) / NAV_LOOKUP_THREADS)),
                       dim3(NAV_LOOKUP_THREADS), 0, (hipStream_t)stream, dist, nav_pitch(dist_pitch, width, height), n_envs,
                       width, height, nav_f2(pos), M, out);
    return tw_launched(__func__);
}

extern "C" int mg_nav_optimal_moves(const uint16_t *dist, int64_t dist_pitch, int n_envs, int width, int height,
                                    const float *pos, const int32_t *age, const float *init_pos, int T, uint8_t *moves,
                                    uint16_t *acting_dist, void *stream)
{
    const int64_t M = (int64_t)T * n_envs;
    if (!nav_field_ok(dist, dist_pitch, n_envs, width, height, true) || !nav_rollout_ok(pos, T) ||
        !nav_clock_ok(age, init_pos, false) || !nav_moves_out_ok(moves, acting_dist) || !nav_count_ok(M))
        return TW_E_ARG;
    if (M == 0) return TW_OK;
    hipLaunchKernelGGL(mg_nav_moves_kernel<false>, nav_grid(M, NAV_MOVES_ELEMS), dim3(NAV_MOVES_THREADS), 0,
                       (hipStream_t)stream, dist, nav_pitch(dist_pitch, width, height), 1, n_envs, width, height,
                       nav_f2(pos), age, init_pos, M, moves, acting_dist);
    return tw_launched(__func__);
}

extern "C" int mg_nav_goal_moves(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                                 uint32_t pass_types, int flags, const int32_t *rec_t, const int32_t *rec_n,
                                 const float *rec_goal, int64_t n_records, const float *pos, const int32_t *age,
                                 const float *init_pos, int T, uint8_t *moves, uint16_t *acting_dist, void *stream)
{
    if (!nav_record_launch_ok(type, n_envs, width, height, pass_types, flags, MG_NAV_DOORS_OPEN, false, nullptr, 0, 1, rec_t,
                              rec_n, rec_goal, n_records, pos, pos, age, init_pos, T) ||
        !nav_moves_out_ok(moves, acting_dist))
        return TW_E_ARG;
    if (n_records == 0) return TW_OK;
    hipLaunchKernelGGL(mg_nav_goal_kernel, nav_grid(n_records, NAV_GOAL_ELEMS), dim3(NAV_GOAL_THREADS), 0,
                       (hipStream_t)stream, type, state, n_envs, width, height, pass_types, flags & MG_NAV_DOORS_OPEN,
                       rec_t, rec_n, rec_goal, n_records, nav_f2(pos), age, init_pos, T, moves, acting_dist);
    return tw_launched(__func__);
}

extern "C" int mg_nav_timed_field(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                                  uint32_t pass_types, int flags, const uint32_t *blocked, int64_t blocked_env_stride,
                                  int period, const int32_t *goal_x, const int32_t *goal_y, int goal_stride,
                                  const int32_t *agent_x, const int32_t *agent_y, const int32_t *agent_clock,
                                  int agent_stride, uint16_t *dist, int64_t dist_pitch, int32_t *agent_dist,
                                  int32_t *agent_action, int32_t *error, void *stream)
{
    if (!nav_world_ok(type, n_envs, width, height, pass_types, flags, MG_NAV_DOORS_OPEN) ||
        !nav_schedule_ok(blocked, blocked_env_stride, period, height) ||
        !nav_field_ok(dist, dist_pitch, n_envs, width, height, false) ||
        !nav_agents_ok(goal_x, goal_y, goal_stride, agent_x, agent_y, agent_stride, agent_dist || agent_action || agent_clock))
        return TW_E_ARG;
    const int HW = width * height, envs = nav_timed_envs(HW, period);
    hipLaunchKernelGGL(nav_period_kernel(period, [](auto p) { return &mg_nav_timed_field_kernel<decltype(p)::value>; }),
                       dim3((n_envs + envs - 1) / envs), dim3(32 * envs), nav_timed_bytes(envs, HW, period), (hipStream_t)stream, type, state, n_envs, width, height,
                       pass_types, flags & MG_NAV_DOORS_OPEN, blocked, blocked_env_stride, goal_x, goal_y, goal_stride,
                       agent_x, agent_y, agent_clock, agent_stride, dist, nav_pitch(dist_pitch, width, height), agent_dist,
                       agent_action, error);
    return tw_launched(__func__);
}

extern "C" int mg_nav_timed_moves(const uint16_t *dist, int64_t dist_pitch, int period, int n_envs, int width, int height,
                                  const float *pos, const int32_t *age, const float *init_pos, int T, uint8_t *moves,
                                  uint16_t *acting_dist, void *stream)
{
    const int64_t M = (int64_t)T * n_envs;
    if (!nav_rollout_launch_ok(dist, dist_pitch, period, n_envs, width, height, pos, pos, age, init_pos, true, T) ||
        !nav_moves_out_ok(moves, acting_dist))
        return TW_E_ARG;
    if (M == 0) return TW_OK;
    hipLaunchKernelGGL(mg_nav_moves_kernel<true>, nav_grid(M, NAV_MOVES_ELEMS), dim3(NAV_MOVES_THREADS), 0,
                       (hipStream_t)stream, dist, nav_pitch(dist_pitch, width, height), period, n_envs, width, height,
                       nav_f2(pos), age, init_pos, M, moves, acting_dist);
    return tw_launched(__func__);
}

extern "C" int mg_nav_timed_goal_floods(int width, int height, int period)
{
    return nav_floods_query(NAV_TIMED_GOAL_LDS, width, height, period);
}

extern "C" int mg_nav_timed_goal_moves(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                                       uint32_t pass_types, int flags, const uint32_t *blocked,
                                       int64_t blocked_env_stride, int period, const int32_t *rec_t, const int32_t *rec_n,
                                       const float *rec_goal, int64_t n_records, const float *pos, const int32_t *age,
                                       const float *init_pos, int T, uint8_t *moves, uint16_t *acting_dist, void *stream)
{
    if (!nav_record_launch_ok(type, n_envs, width, height, pass_types, flags, MG_NAV_DOORS_OPEN, true, blocked,
                              blocked_env_stride, period, rec_t, rec_n, rec_goal, n_records, pos, pos, age, init_pos, T) ||
        !nav_moves_out_ok(moves, acting_dist))
        return TW_E_ARG;
    if (n_records == 0) return TW_OK;
    const int HW = width * height, flooders = nav_timed_goal_flooders(NAV_TIMED_GOAL_LDS, HW, period);
    hipLaunchKernelGGL(nav_period_kernel(period, [](auto p) { return &mg_nav_timed_goal_kernel<decltype(p)::value>; }), nav_grid(n_records, NAV_GOAL_ELEMS), dim3(NAV_GOAL_THREADS),
                       nav_timed_bytes(flooders, HW, period), (hipStream_t)stream, type, state, n_envs, width, height,
                       pass_types, flags & MG_NAV_DOORS_OPEN, blocked, blocked_env_stride, rec_t, rec_n, rec_goal,
                       n_records, nav_f2(pos), age, init_pos, T, moves, acting_dist, flooders);
    return tw_launched(__func__);
}

extern "C" int mg_nav_shape(const uint16_t *dist, int64_t dist_pitch, int period, int n_envs, int width, int height,
                            const float *pos_before, const float *pos_after, const int32_t *age, const float *init_pos,
                            const uint8_t *done, const float *reward, int T, float scale, float gamma, int flags,
                            float *reward_out, float *shaping, uint8_t *mask, void *stream)
{
    const int64_t M = (int64_t)T * n_envs;
    if (!nav_rollout_launch_ok(dist, dist_pitch, period, n_envs, width, height, pos_before, pos_after, age, init_pos,
                               period > 1, T) ||
        !nav_flags_ok(flags, MG_NAV_SHAPE_ZERO_TERMINAL) ||     // no MG_NAV_DOORS_OPEN: the doors are the field's business
        !nav_shaping_ok(reward, done, flags, scale, gamma, reward_out, shaping, mask))
        return TW_E_ARG;
    if (M == 0) return TW_OK;
    hipLaunchKernelGGL(period > 1 ? mg_nav_shape_kernel<true> : mg_nav_shape_kernel<false>, nav_grid(M, NAV_MOVES_ELEMS),
                       dim3(NAV_MOVES_THREADS), 0, (hipStream_t)stream, dist, nav_pitch(dist_pitch, width, height), period,
                       n_envs, width, height, nav_f2(pos_before), nav_f2(pos_after), age, init_pos, nav_ends(done, flags),
                       reward, M, scale, gamma, reward_out, shaping, mask);
    return tw_launched(__func__);
}

extern "C" int mg_nav_goal_shape(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                                 uint32_t pass_types, int flags, const int32_t *rec_t, const int32_t *rec_n,
                                 const float *rec_goal, const uint8_t *rec_done, const float *rec_reward,
                                 int64_t n_records, const float *pos_before, const float *pos_after, const int32_t *age,
                                 const float *init_pos, int T, float scale, float gamma, float *reward_out, float *shaping,
                                 uint8_t *mask, void *stream)
{
    if (!nav_record_launch_ok(type, n_envs, width, height, pass_types, flags, MG_NAV_DOORS_OPEN | MG_NAV_SHAPE_ZERO_TERMINAL,
                              false, nullptr, 0, 1, rec_t, rec_n, rec_goal, n_records, pos_before, pos_after, age, init_pos, T) ||
        !nav_shaping_ok(rec_reward, rec_done, flags, scale, gamma, reward_out, shaping, mask))
        return TW_E_ARG;
    if (n_records == 0) return TW_OK;
    hipLaunchKernelGGL(mg_nav_goal_shape_kernel, nav_grid(n_records, NAV_GOAL_ELEMS), dim3(NAV_GOAL_THREADS), 0,
                       (hipStream_t)stream, type, state, n_envs, width, height, pass_types, flags & MG_NAV_DOORS_OPEN,
                       rec_t, rec_n, rec_goal, nav_ends(rec_done, flags), rec_reward, n_records, nav_f2(pos_before),
                       nav_f2(pos_after), age, init_pos, T, scale, gamma, reward_out, shaping, mask);
    return tw_launched(__func__);
}

extern "C" int mg_nav_timed_goal_shape_floods(int width, int height, int period)
{
    return nav_floods_query(MG_NAV_TIMED_GOAL_SHAPE_LDS, width, height, period);
}

extern "C" int mg_nav_timed_goal_shape(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                                       uint32_t pass_types, int flags, const uint32_t *blocked,
                                       int64_t blocked_env_stride, int period, const int32_t *rec_t, const int32_t *rec_n,
                                       const float *rec_goal, const uint8_t *rec_done, const float *rec_reward,
                                       int64_t n_records, const float *pos_before, const float *pos_after,
                                       const int32_t *age, const float *init_pos, int T, float scale, float gamma,
                                       float *reward_out, float *shaping, uint8_t *mask, void *stream)
{
    if (!nav_record_launch_ok(type, n_envs, width, height, pass_types, flags, MG_NAV_DOORS_OPEN | MG_NAV_SHAPE_ZERO_TERMINAL,
                              true, blocked, blocked_env_stride, period, rec_t, rec_n, rec_goal, n_records, pos_before,
                              pos_after, age, init_pos, T) ||
        !nav_shaping_ok(rec_reward, rec_done, flags, scale, gamma, reward_out, shaping, mask))
        return TW_E_ARG;
    if (n_records == 0) return TW_OK;
    const int HW = width * height, flooders = nav_timed_goal_flooders(MG_NAV_TIMED_GOAL_SHAPE_LDS, HW, period);
    hipLaunchKernelGGL(nav_period_kernel(period, [](auto p) { return &mg_nav_timed_goal_shape_kernel<decltype(p)::value>; }), nav_grid(n_records, NAV_GOAL_ELEMS), dim3(NAV_GOAL_THREADS),
                       nav_timed_bytes(flooders, HW, period), (hipStream_t)stream, type, state, n_envs, width, height,
                       pass_types, flags & MG_NAV_DOORS_OPEN, blocked, blocked_env_stride, rec_t, rec_n, rec_goal,
                       nav_ends(rec_done, flags), rec_reward, n_records, nav_f2(pos_before), nav_f2(pos_after), age,
                       init_pos, T, scale, gamma, reward_out, shaping, mask, flooders);
    return tw_launched(__func__);
}

extern "C" int mg_nav_ahead(const uint16_t *dist, int64_t dist_pitch, int period, int n_envs, int width, int height,
                            const float *pos, const int32_t *age, const float *init_pos, int T, int steps, uint64_t *ahead,
                            uint16_t *acting_dist, void *stream)
{
    const int64_t M = (int64_t)T * n_envs;
    if (!nav_rollout_launch_ok(dist, dist_pitch, period, n_envs, width, height, pos, pos, age, init_pos, period > 1, T) ||
        !nav_ahead_out_ok(steps, ahead, acting_dist))
        return TW_E_ARG;
    if (M == 0) return TW_OK;
    hipLaunchKernelGGL(period > 1 ? mg_nav_ahead_kernel<true> : mg_nav_ahead_kernel<false>, nav_grid(M, NAV_MOVES_ELEMS),
                       dim3(NAV_MOVES_THREADS), 0, (hipStream_t)stream, dist, nav_pitch(dist_pitch, width, height), period,
                       n_envs, width, height, nav_f2(pos), age, init_pos, M, steps,
                       reinterpret_cast<unsigned long long *>(ahead), acting_dist);
    return tw_launched(__func__);
}

extern "C" int mg_nav_goal_ahead(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                                 uint32_t pass_types, int flags, const int32_t *rec_t, const int32_t *rec_n,
                                 const float *rec_goal, int64_t n_records, const float *pos, const int32_t *age,
                                 const float *init_pos, int T, int steps, uint64_t *ahead, uint16_t *acting_dist,
                                 void *stream)
{
    if (!nav_record_launch_ok(type, n_envs, width, height, pass_types, flags, MG_NAV_DOORS_OPEN, false, nullptr, 0, 1, rec_t,
                              rec_n, rec_goal, n_records, pos, pos, age, init_pos, T) ||
        !nav_ahead_out_ok(steps, ahead, acting_dist))
        return TW_E_ARG;
    if (n_records == 0) return TW_OK;
    hipLaunchKernelGGL(mg_nav_goal_ahead_kernel, nav_grid(n_records, NAV_GOAL_ELEMS), dim3(NAV_GOAL_THREADS), 0,
                       (hipStream_t)stream, type, state, n_envs, width, height, pass_types, flags & MG_NAV_DOORS_OPEN,
                       rec_t, rec_n, rec_goal, n_records, nav_f2(pos), age, init_pos, T, steps,
                       reinterpret_cast<unsigned long long *>(ahead), acting_dist);
    return tw_launched(__func__);
}

extern "C" int mg_nav_timed_goal_ahead_floods(int width, int height, int period)
{
    return nav_floods_query(MG_NAV_TIMED_GOAL_AHEAD_LDS, width, height, period);
}

extern "C" int mg_nav_timed_goal_ahead(const uint8_t *type, const uint8_t *state, int n_envs, int width, int height,
                                       uint32_t pass_types, int flags, const uint32_t *blocked,
                                       int64_t blocked_env_stride, int period, const int32_t *rec_t, const int32_t *rec_n,
                                       const float *rec_goal, int64_t n_records, const float *pos, const int32_t *age,
                                       const float *init_pos, int T, int steps, uint64_t *ahead, uint16_t *acting_dist,
                                       void *stream)
{
    if (!nav_record_launch_ok(type, n_envs, width, height, pass_types, flags, MG_NAV_DOORS_OPEN, true, blocked,
                              blocked_env_stride, period, rec_t, rec_n, rec_goal, n_records, pos, pos, age, init_pos, T) ||
        !nav_ahead_out_ok(steps, ahead, acting_dist))
        return TW_E_ARG;
    if (n_records == 0) return TW_OK;
    const int HW = width * height, flooders = nav_timed_goal_flooders(MG_NAV_TIMED_GOAL_AHEAD_LDS, HW, period);
    hipLaunchKernelGGL(nav_period_kernel(period, [](auto p) { return &mg_nav_timed_goal_ahead_kernel<decltype(p)::value>; }),
                       nav_grid(n_records, NAV_GOAL_ELEMS), dim3(NAV_GOAL_THREADS), nav_timed_bytes(flooders, HW, period),
                       (hipStream_t)stream, type, state, n_envs, width, height, pass_types, flags & MG_NAV_DOORS_OPEN, blocked,
                       blocked_env_stride, rec_t, rec_n, rec_goal, n_records, nav_f2(pos), age, init_pos, T, steps,
                       reinterpret_cast<unsigned long long *>(ahead), acting_dist, flooders);
    return tw_launched(__func__);
}

extern "C" int mg_nav_path_scan(const uint16_t *dist, int64_t dist_pitch, int period, int n_envs, int width, int height,
                                const float *pos_before, const float *pos_after, const int32_t *age, const float *init_pos,
                                const uint8_t *terminated, const uint8_t *truncated, int T, uint16_t *carry_start,
                                uint16_t *carry_best, int32_t *carry_off, int32_t *carry_steps, uint16_t *ep_start,
                                uint16_t *ep_best, int32_t *ep_off, int32_t *ep_steps, void *stream)
{
    const int64_t M = (int64_t)T * n_envs;
    if (!nav_rollout_launch_ok(dist, dist_pitch, period, n_envs, width, height, pos_before, pos_after, age, init_pos,
                               period > 1, T) ||
        !nav_flags_given(terminated, truncated) || !nav_path_arrays_ok(carry_start, carry_best, carry_off, carry_steps, true) ||
        !nav_path_arrays_ok(ep_start, ep_best, ep_off, ep_steps, false))
        return TW_E_ARG;
    if (M == 0) return TW_OK;
    hipLaunchKernelGGL(period > 1 ? mg_nav_path_scan_kernel<true> : mg_nav_path_scan_kernel<false>,
                       dim3((n_envs + NAV_PATH_THREADS - 1) / NAV_PATH_THREADS), dim3(NAV_PATH_THREADS), 0,
                       (hipStream_t)stream, dist, nav_pitch(dist_pitch, width, height), period, n_envs, width, height,
                       nav_f2(pos_before), nav_f2(pos_after), age, init_pos, terminated, truncated, T, carry_start,
                       carry_best, carry_off, carry_steps, ep_start, ep_best, ep_off, ep_steps);
    return tw_launched(__func__);
}

extern "C" int mg_nav_path_summary_workspace(int T, int N)
{
    if (T <= 0 || N <= 0 || !nav_count_ok((int64_t)T * N)) return TW_E_ARG;
    return nav_path_blocks((int64_t)T * N) * NAV_PATH_NV;
}

extern "C" int mg_nav_path_summary(const uint16_t *ep_start, const uint16_t *ep_best, const int32_t *ep_off,
                                   const int32_t *ep_steps, const uint8_t *terminated, const uint8_t *truncated, int T, int N,
                                   double *summary, double *workspace, void *stream)
{
    const int64_t M = (int64_t)T * N;
    if (!nav_path_arrays_ok(ep_start, ep_best, ep_off, ep_steps, true) || !nav_flags_given(terminated, truncated) ||
        T <= 0 || N <= 0 || !nav_count_ok(M) || !summary || !workspace || !nav_aligned(summary, 8) ||
        !nav_aligned(workspace, 8))
        return TW_E_ARG;
    const int nblocks = nav_path_blocks(M);
    const int64_t per_block = (M + nblocks - 1) / nblocks;
    const int per_thread = (int)((per_block + NAV_PATH_SUM_THREADS - 1) / NAV_PATH_SUM_THREADS);
    hipLaunchKernelGGL(mg_nav_path_partial_kernel, dim3(nblocks), dim3(NAV_PATH_SUM_THREADS), 0, (hipStream_t)stream,
                       ep_start, ep_best, ep_off, ep_steps, terminated, truncated, M, per_block, per_thread, workspace);
    hipLaunchKernelGGL(mg_nav_path_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, workspace, nblocks, summary);
    return tw_launched(__func__);
}
