"""Torch front end of the shortest-path kernels (include/minigrid_nav.h, csrc/minigrid_nav.hip): how many moves every cell
of N grid worlds lies from the goal, and which of mg_step's four moves an agent on a shortest path makes next.  World planes
are uint8[N, H*W] with cell (x, y) at y*W + x; goal and agent coordinates are int32[N] tensors, dense or the column views
of the engine's records (TwoarmyEngine.agent_views()), read where they live.  goal_moves labels records that each name a
goal of their own (hindsight records) without a field in memory.  timed_field / timed_moves do the same for worlds whose
blockers move with a period (a search over (cell, phase): the expert may wait).  shape / goal_shape / timed_goal_shape turn
the distances into a potential and shape rewards with it, float32 with pinned rounding.  ahead / goal_ahead /
timed_goal_ahead say where a shortest path leads in up to three steps, as a set of displacements.  path_scan / path_summary / PathTracker
rate every episode against the field: success weighted by path length, progress, steps off a shortest path.  One launch per
call (path_summary: two), on the tensors' device.
No CPU fallback."""
import ctypes

import torch

from ._marshal import agent_arrays, call, inner, ptr, query, rows

MAX_SIDE = 32
MAX_PERIOD = 16                       # timed_field: phases of a schedule
UNREACHABLE = 0xFFFF
PASS_DEFAULT = 0x0B1B                 # mg_step's rule: types 0, 1, 3, 8, 9, 11 and open doors (bit 4)
PASS_LAVA, PASS_BALL = 1 << 9, 1 << 6  # clear PASS_LAVA to keep out of the lava, set PASS_BALL to walk through balls
DOORS_OPEN = 1
SHAPE_ZERO_TERMINAL = 2               # shape / goal_shape: phi(after) = 0 where the step ended its episode
ACTION_STAY, ACTION_NONE = 6, -1
MOVE_STAY = 1 << 4                    # optimal_moves: the bit of a source cell (bits 0..3: left, right, up, down)


DIST_DTYPE = torch.uint16


def _planes(type_plane, state, width, height):
    """(N, W, H, device) of the world planes uint8[N, H*W]."""
    N, W, H = type_plane.shape[0], int(width), int(height)
    assert type_plane.shape == (N, W * H)
    assert state is None or state.shape == (N, W * H)
    return N, W, H, type_plane.device


def _records(rec_t, rec_n, rec_goal, dev):
    """R of the records t[R], n[R], goal[R, 2]."""
    R = rec_t.shape[0]
    assert rec_t.shape == (R,) and rec_n.shape == (R,) and rec_goal.shape == (R, 2), "expected t[R], n[R], goal[R, 2]"
    assert rec_t.device == dev and rec_n.device == dev and rec_goal.device == dev
    return R


def _positions(N, dev, *pos):
    """T of one or two rollout position tensors float32[T, N, 2]."""
    for p in pos:
        assert p.dtype == torch.float32 and p.dim() == 3 and p.is_contiguous() and p.shape[1:] == (N, 2) and p.device == dev
    T = pos[0].shape[0]
    assert pos[-1].shape[0] == T
    return T


def _clock(age, init_pos, T, N, dev, required=False):
    """age int32[T, N] comes with init_pos float32[2]; required: the age is the clock of a timed field."""
    if required:
        assert age is not None and init_pos is not None, "the age is the clock: age and init_pos are required"
    else:
        assert (age is None) == (init_pos is None), "age and init_pos come together"
    if age is not None:
        assert age.shape == (T, N) and age.device == dev and init_pos.shape == (2,) and init_pos.device == dev


def _moves_outputs(shape, dev, dtype, out, dist_out):
    """(out, dist_out) of a launch that labels with `dtype` (move sets uint8, look-ahead labels AHEAD_DTYPE): None = a new
    tensor, dist_out False = no distances (None is returned)."""
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    assert out.shape == shape and out.device == dev
    if dist_out is None:
        dist_out = torch.empty(shape, dtype=DIST_DTYPE, device=dev)
    elif dist_out is False:
        dist_out = None
    assert dist_out is None or (dist_out.shape == shape and dist_out.device == dev)
    return out, dist_out


def _timed_rows(dist, W, H):
    """(pointer, pitch in elements, N, P) of fields uint16[N, P, H*W] whose rows are dense but may be padded."""
    assert dist.is_cuda and dist.dtype == DIST_DTYPE and dist.dim() == 3 and dist.shape[2] == W * H
    N, P = dist.shape[0], dist.shape[1]
    inner(dist, 2)
    dpitch = dist.stride(1) if P > 1 else (dist.stride(0) if N > 1 else W * H)
    assert dpitch >= W * H and (N == 1 or dist.stride(0) == P * dpitch), "expected rows of one pitch, P per env"
    return ctypes.c_void_p(dist.data_ptr()), int(dpitch), N, P


def _field_rows(field, W, H):
    """(pointer, pitch in elements, N, P) of a static field uint16[N, H*W] or a timed one uint16[N, P, H*W]."""
    if field.dim() == 3:
        return _timed_rows(field, W, H)
    dp, dpitch, N, row = rows(field, DIST_DTYPE)
    assert row == W * H
    return dp, dpitch, N, 1


def _launch(name, dev, count, outs, args):
    """lib.<name>(*args()) over `count` elements or records -> outs.  count = 0: empty tensors have no address to hand over,
    and there is nothing to launch, so args() is not even formed."""
    if count:
        call(name, dev, *args())
    return outs


def _record_args(type_plane, state, width, height, pass_types, flags, blocked, rec_t, rec_n, rec_goal, pos, age, init_pos):
    """What every record call marshals: the planes, the schedule (blocked None: the static map, the clock optional; else the
    age is the clock and required), the records, one or two position tensors `pos` and the clock.
    -> (head, tail, (N, W, H, R, T, P, dev)): head() = the C arguments up to rec_goal, tail() = those from the record count
    to T; a call is head(), what the kind adds of a record, tail(), then scalars and outputs."""
    N, W, H, dev = _planes(type_plane, state, width, height)
    sched, P = (), 1
    if blocked is not None:
        sched = _schedule(blocked, N, H, dev)
        P = sched[2]
    R = _records(rec_t, rec_n, rec_goal, dev)
    T = _positions(N, dev, *pos)
    _clock(age, init_pos, T, N, dev, required=blocked is not None)

    def head():
        return (ptr(type_plane, torch.uint8), ptr(state, torch.uint8), N, W, H, int(pass_types), flags, *sched,
                ptr(rec_t, torch.int32), ptr(rec_n, torch.int32), ptr(rec_goal, torch.float32))

    def tail():
        return (R, *(ptr(q) for q in pos), ptr(age, torch.int32), ptr(init_pos, torch.float32), T)
    return head, tail, (N, W, H, R, T, P, dev)


def _record_moves(name, blocked, type_plane, rec_t, rec_n, rec_goal, pos, width, height, pass_types, age, init_pos, state,
                  doors_open, out, dist_out):
    """goal_moves / timed_goal_moves."""
    head, tail, (N, W, H, R, T, P, dev) = _record_args(type_plane, state, width, height, pass_types,
                                                       DOORS_OPEN if doors_open else 0, blocked, rec_t, rec_n, rec_goal,
                                                       (pos,), age, init_pos)
    out, dist_out = _moves_outputs((R,), dev, torch.uint8, out, dist_out)
    return _launch(name, dev, R, (out, dist_out),
                   lambda: (*head(), *tail(), ptr(out, torch.uint8), ptr(dist_out, DIST_DTYPE)))


def _record_ahead(name, blocked, type_plane, rec_t, rec_n, rec_goal, pos, width, height, steps, pass_types, age, init_pos,
                  state, doors_open, out, dist_out):
    """goal_ahead / timed_goal_ahead."""
    head, tail, (N, W, H, R, T, P, dev) = _record_args(type_plane, state, width, height, pass_types,
                                                       DOORS_OPEN if doors_open else 0, blocked, rec_t, rec_n, rec_goal,
                                                       (pos,), age, init_pos)
    out, dist_out = _moves_outputs((R,), dev, AHEAD_DTYPE, out, dist_out)
    return _launch(name, dev, R, (out, dist_out),
                   lambda: (*head(), *tail(), int(steps), ptr(out, AHEAD_DTYPE), ptr(dist_out, DIST_DTYPE)))


def _record_shape(name, blocked, type_plane, rec_t, rec_n, rec_goal, pos_before, pos_after, width, height, reward, done,
                  pass_types, age, init_pos, state, doors_open, scale, gamma, zero_terminal, out, shaping_out, mask_out):
    """goal_shape / timed_goal_shape."""
    flags = (DOORS_OPEN if doors_open else 0) | (SHAPE_ZERO_TERMINAL if zero_terminal else 0)
    head, tail, (N, W, H, R, T, P, dev) = _record_args(type_plane, state, width, height, pass_types, flags, blocked, rec_t,
                                                       rec_n, rec_goal, (pos_before, pos_after), age, init_pos)
    assert not zero_terminal or done is not None, "zero_terminal needs done"
    assert done is None or (done.shape == (R,) and done.device == dev)
    outs = _shape_outputs((R,), dev, reward, out, shaping_out, mask_out)
    return _launch(name, dev, R, outs,
                   lambda: (*head(), ptr(done, torch.uint8), ptr(reward, torch.float32), *tail(), float(scale), float(gamma),
                            ptr(outs[0], torch.float32), ptr(outs[1], torch.float32), ptr(outs[2], torch.uint8)))


def distance_field(type_plane, state_plane, width, height, pass_types=PASS_DEFAULT, goal=None, agent=None, out=None,
                   doors_open=False, want_field=True, want_error=True, agent_out=None, error_out=None):
    """-> (dist, agent_dist, agent_action, error).
    dist uint16[N, H*W]: moves to the nearest source through enterable cells, UNREACHABLE elsewhere (`out`: a [N, H*W]
    tensor whose rows may be padded; want_field=False: no field, None is returned).  goal = (x, y) int32[N] tensors, or
    None: every cell of type 8.  agent = (x, y) int32[N] tensors -> agent_dist int32[N] and agent_action int32[N]
    (0 left, 1 right, 2 up, 3 down, 6 stay on a source, -1 unreachable), else None.  error int32[N]: 0 ok, 1 no source,
    2 source outside the world, 3 agent outside the world.  agent_out = (agent_dist, agent_action) and error_out:
    contiguous int32[N] tensors to write into, so that a call per step allocates nothing."""
    N, W, H, dev = _planes(type_plane, state_plane, width, height)
    dp, dpitch = None, 0
    if out is not None or want_field:
        if out is None:
            out = torch.empty((N, W * H), dtype=DIST_DTYPE, device=dev)
        dp, dpitch, No, row = rows(out, DIST_DTYPE)
        assert No == N and row == W * H and out.device == dev
    gx = gy = ax = ay = None
    gstride = astride = 1
    if goal is not None:
        gx, gy, _, gstride = agent_arrays(goal[0], goal[1])
        assert goal[0].shape[0] >= N and goal[0].device == dev
    adist = aact = None
    if agent is not None:
        ax, ay, _, astride = agent_arrays(agent[0], agent[1])
        assert agent[0].shape[0] >= N and agent[0].device == dev
        adist, aact = agent_out if agent_out is not None else (_int32(None, N, dev), _int32(None, N, dev))
        _int32(adist, N, dev), _int32(aact, N, dev)
    else:
        assert agent_out is None, "agent_out without agent"
    err = _int32(error_out, N, dev) if want_error or error_out is not None else None
    call("mg_nav_field", dev, ptr(type_plane, torch.uint8), ptr(state_plane, torch.uint8), N, W, H, int(pass_types),
         DOORS_OPEN if doors_open else 0, gx, gy, gstride, ax, ay, astride, dp, dpitch, ptr(adist), ptr(aact), ptr(err))
    return out, adist, aact, err


def _int32(t, N, dev):
    """t, checked to be a contiguous int32[N] tensor on dev; a new one for None."""
    if t is None:
        return torch.empty(N, dtype=torch.int32, device=dev)
    assert t.shape == (N,) and t.dtype == torch.int32 and t.device == dev and t.is_contiguous(), "expected int32[N] on the planes' device"
    return t


def lookup(dist, pos, width, height, out=None):
    """dist uint16[N, H*W] (one field per env, rows may be padded), pos float32[T, N, 2] = (y, x) after each step (or
    [N, 2]: one step) -> uint16[T, N] ([N]): the distance of the cell each position lies in by the rule of the visit
    counters, UNREACHABLE for a position outside the world."""
    W, H = int(width), int(height)
    dp, dpitch, N, row = rows(dist, DIST_DTYPE)
    assert row == W * H
    one = pos.dim() == 2
    p = pos.view(1, -1, 2) if one else pos
    assert p.dtype == torch.float32 and p.is_contiguous() and p.shape[1:] == (N, 2) and p.device == dist.device
    T = p.shape[0]
    if out is None:
        out = torch.empty((T, N), dtype=DIST_DTYPE, device=dist.device)
    assert out.shape == (T, N) and out.dtype == DIST_DTYPE
    call("mg_nav_lookup", dist.device, dp, dpitch, N, W, H, ptr(p), T, ptr(out))
    return out.view(N) if one else out


def optimal_moves(dist, pos, width, height, age=None, init_pos=None, out=None, dist_out=None):
    """The set of optimal moves at every acting state of a rollout (mg_nav_optimal_moves, include/minigrid_nav.h).
    dist uint16[N, H*W] (one field per env, rows may be padded), pos float32[T, N, 2] = (y, x) BEFORE each step, age
    int32[T, N] with init_pos float32[2]: where age <= 0 the acting position is init_pos (ppo_gather_stack's rule); both
    None: pos as it stands.  -> (moves uint8[T, N], acting_dist uint16[T, N]): bit k of moves = move k (left, right, up,
    down) leads one step nearer, MOVE_STAY on a source, 0 on an unreachable cell or outside the world.  out / dist_out:
    tensors to write into; dist_out=False: no distances (None is returned for them).  One launch."""
    W, H = int(width), int(height)
    dp, dpitch, N, row = rows(dist, DIST_DTYPE)
    assert row == W * H
    dev = dist.device
    T = _positions(N, dev, pos)
    _clock(age, init_pos, T, N, dev)
    out, dist_out = _moves_outputs((T, N), dev, torch.uint8, out, dist_out)
    call("mg_nav_optimal_moves", dev, dp, dpitch, N, W, H, ptr(pos), ptr(age, torch.int32), ptr(init_pos, torch.float32), T,
         ptr(out, torch.uint8), ptr(dist_out, DIST_DTYPE))
    return out, dist_out


def goal_moves(type_plane, rec_t, rec_n, rec_goal, pos, width, height, pass_types=PASS_DEFAULT, age=None, init_pos=None,
               state=None, doors_open=False, out=None, dist_out=None):
    """The set of optimal moves of records that each name their own goal (mg_nav_goal_moves, include/minigrid_nav.h):
    type_plane (state) uint8[N, H*W] as distance_field takes them; rec_t, rec_n int32[R] and rec_goal float32[R, 2] =
    (y, x), the t, n and goal of ppo_ops.her_relabel's records; pos float32[T, N, 2], age int32[T, N] and init_pos
    float32[2] as optimal_moves takes them.  -> (moves uint8[R], acting_dist uint16[R]): per record what optimal_moves
    gives in the field of the record's env flooded from the record's goal cell; 0 / UNREACHABLE for a record whose t,
    n, goal or acting position names nothing.  out / dist_out: tensors to write into; dist_out=False: no distances
    (None is returned for them).  One launch (none for R = 0), no host synchronisation."""
    return _record_moves("mg_nav_goal_moves", None, type_plane, rec_t, rec_n, rec_goal, pos, width, height, pass_types, age,
                         init_pos, state, doors_open, out, dist_out)


def _schedule(blocked, N, H, dev):
    """(pointer, env stride in words, P) of a schedule tensor: int32 / uint32 [P, H] (shared) or [N, P, H] (per env)."""
    assert blocked.dtype in (torch.int32, torch.uint32) and blocked.is_cuda and blocked.device == dev, \
        "expected a 32-bit schedule on the planes' device"
    assert blocked.dim() in (2, 3) and blocked.shape[-1] == H and blocked.is_contiguous(), "expected [P, H] or [N, P, H]"
    P = blocked.shape[-2]
    assert 1 <= P <= MAX_PERIOD and (blocked.dim() == 2 or blocked.shape[0] == N)
    return ptr(blocked), (0 if blocked.dim() == 2 else P * H), P


def timed_field(type_plane, state_plane, width, height, blocked, pass_types=PASS_DEFAULT, goal=None, agent=None,
                clock=None, out=None, doors_open=False, want_field=True, want_error=True, agent_out=None, error_out=None):
    """distance_field for a world whose blockers move with a period (mg_nav_timed_field, include/minigrid_nav.h)
    -> (dist, agent_dist, agent_action, error).
    blocked: int32 / uint32 [P, H] (one schedule for all envs) or [N, P, H]: bit x of word y of phase p = cell (x, y) is
    occupied at phase p.  dist uint16[N, P, H*W]: transitions (a move or a wait, the phase advancing by one) from (cell,
    phase) to the nearest source, UNREACHABLE where the cell is not free at that phase or no path exists (`out`: a
    [N, P, H*W] tensor whose rows may be padded; want_field=False: None).  agent = (x, y) int32[N] with clock int32[N]
    sharing their stride (None: phase 0): the agent's phase is clock <= 0 ? 0 : clock % P.  agent_action: 0..3 a move, 6
    stay on a source OR wait for the blockers, -1 unreachable.  Everything else as distance_field takes and returns it."""
    N, W, H, dev = _planes(type_plane, state_plane, width, height)
    bp, bstride, P = _schedule(blocked, N, H, dev)
    dp, dpitch = None, 0
    if out is not None or want_field:
        if out is None:
            out = torch.empty((N, P, W * H), dtype=DIST_DTYPE, device=dev)
        dp, dpitch, No, Po = _timed_rows(out, W, H)
        assert (No, Po) == (N, P) and out.device == dev
    gx = gy = ax = ay = cp = None
    gstride = astride = 1
    if goal is not None:
        gx, gy, _, gstride = agent_arrays(goal[0], goal[1])
        assert goal[0].shape[0] >= N and goal[0].device == dev
    adist = aact = None
    if agent is not None:
        ax, ay, cp, astride = agent_arrays(agent[0], agent[1], clock)
        assert agent[0].shape[0] >= N and agent[0].device == dev
        adist, aact = agent_out if agent_out is not None else (_int32(None, N, dev), _int32(None, N, dev))
        _int32(adist, N, dev), _int32(aact, N, dev)
    else:
        assert agent_out is None and clock is None, "agent_out or clock without agent"
    err = _int32(error_out, N, dev) if want_error or error_out is not None else None
    call("mg_nav_timed_field", dev, ptr(type_plane, torch.uint8), ptr(state_plane, torch.uint8), N, W, H, int(pass_types),
         DOORS_OPEN if doors_open else 0, bp, bstride, P, gx, gy, gstride, ax, ay, cp, astride, dp, dpitch, ptr(adist),
         ptr(aact), ptr(err))
    return out, adist, aact, err


def timed_moves(dist, pos, width, height, age, init_pos, out=None, dist_out=None):
    """optimal_moves for a timed field (mg_nav_timed_moves, include/minigrid_nav.h): dist uint16[N, P, H*W] as
    timed_field returns it (rows may be padded), pos float32[T, N, 2] = (y, x) BEFORE each step, age int32[T, N] (the
    clock as well: the phase of (t, n) is age <= 0 ? 0 : age % P) and init_pos float32[2], both required.
    -> (moves uint8[T, N], acting_dist uint16[T, N]): bits 0..3 = the move leads one transition nearer, MOVE_STAY = on a
    source, or waiting is optimal; 0 on an unreachable state or outside the world.  out / dist_out as in optimal_moves."""
    W, H = int(width), int(height)
    dp, dpitch, N, P = _timed_rows(dist, W, H)
    dev = dist.device
    T = _positions(N, dev, pos)
    _clock(age, init_pos, T, N, dev, required=True)
    out, dist_out = _moves_outputs((T, N), dev, torch.uint8, out, dist_out)
    return _launch("mg_nav_timed_moves", dev, T, (out, dist_out),
                   lambda: (dp, dpitch, P, N, W, H, ptr(pos), ptr(age, torch.int32), ptr(init_pos, torch.float32), T,
                            ptr(out, torch.uint8), ptr(dist_out, DIST_DTYPE)))


def timed_goal_moves(type_plane, rec_t, rec_n, rec_goal, pos, width, height, blocked, age, init_pos,
                     pass_types=PASS_DEFAULT, state=None, doors_open=False, out=None, dist_out=None):
    """goal_moves for a world whose blockers move with a period (mg_nav_timed_goal_moves, include/minigrid_nav.h): the
    planes, the records (rec_t, rec_n int32[R], rec_goal float32[R, 2] = (y, x)) and pos float32[T, N, 2] as goal_moves
    takes them, blocked int32 / uint32 [P, H] or [N, P, H] as timed_field takes it, age int32[T, N] (the clock as well: the
    phase of a record is age[t, n] <= 0 ? 0 : age[t, n] % P) and init_pos float32[2], both required.
    -> (moves uint8[R], acting_dist uint16[R]): per record what timed_moves gives in the time-expanded field of the
    record's env flooded from the record's goal cell -- bits 0..3 = the move leads one transition nearer, MOVE_STAY = on
    the goal, or waiting is optimal; 0 / UNREACHABLE for a record whose t, n, goal or acting position names nothing,
    whose goal cell is free at no phase or whose state has no path.  out / dist_out as in goal_moves.  One launch (none
    for R = 0), no field in memory, no host synchronisation."""
    return _record_moves("mg_nav_timed_goal_moves", blocked, type_plane, rec_t, rec_n, rec_goal, pos, width, height,
                         pass_types, age, init_pos, state, doors_open, out, dist_out)


def timed_goal_floods(width, height, period):
    """How many of a workgroup's 8 half wavefronts flood at a time in timed_goal_moves at this size and period (8, 4, 2
    or 1: their images share 64 KiB of LDS with the staging) -- the launch's own host function."""
    return query("mg_nav_timed_goal_floods", int(width), int(height), int(period))


def _shape_outputs(shape, dev, reward, out, shaping_out, mask_out):
    """The three outputs of shape / goal_shape: None = a new tensor (out: only with a reward), False = not wanted, a tensor
    = written into (out may be `reward` itself: in place).  -> (out, shaping, mask), None where not wanted."""
    if reward is not None:
        assert reward.shape == shape and reward.device == dev and reward.dtype == torch.float32
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev) if reward is not None else False
    shaping_out = torch.empty(shape, dtype=torch.float32, device=dev) if shaping_out is None else shaping_out
    mask_out = torch.empty(shape, dtype=torch.uint8, device=dev) if mask_out is None else mask_out
    res = tuple(None if t is False else t for t in (out, shaping_out, mask_out))
    assert res[0] is None or reward is not None, "out without a reward"
    assert any(t is not None for t in res), "no output wanted"
    assert all(t is None or (t.shape == shape and t.device == dev) for t in res)
    return res


def shape(dist, pos_before, pos_after, width, height, reward=None, age=None, init_pos=None, done=None, scale=1.0,
          gamma=0.99, zero_terminal=False, out=None, shaping_out=None, mask_out=None):
    """Potential-based reward shaping of a rollout from one field per env (mg_nav_shape, include/minigrid_nav.h):
    out = reward + F, F = gamma * phi(after) - phi(before), phi = -scale * distance, float32 with one rounding per
    operation.  dist uint16[N, H*W] as distance_field returns it or uint16[N, P, H*W] as timed_field does (the period is
    dist's second dimension; rows may be padded); pos_before, pos_after float32[T, N, 2] = (y, x) before / after each step,
    age int32[T, N] with init_pos float32[2] as optimal_moves takes them (required with a timed field: the age is the
    clock); reward float32[T, N] or None; done uint8[T, N], required with zero_terminal=True (phi(after) = 0 where done).
    -> (out float32[T, N], F float32[T, N], mask uint8[T, N]): mask 0 where either state is no cell or unreachable -- there
    F = 0 and the reward passes through bit for bit.  out / shaping_out / mask_out: tensors to write into (out=reward
    shapes in place), False: not wanted (None is returned for it); out needs a reward.  One launch (none for T = 0)."""
    W, H = int(width), int(height)
    dp, dpitch, N, P = _field_rows(dist, W, H)
    dev = dist.device
    T = _positions(N, dev, pos_before, pos_after)
    _clock(age, init_pos, T, N, dev)
    assert age is not None or P == 1, "the age is the clock: age and init_pos are required with a timed field"
    assert not zero_terminal or done is not None, "zero_terminal needs done"
    assert done is None or (done.shape == (T, N) and done.device == dev)
    outs = _shape_outputs((T, N), dev, reward, out, shaping_out, mask_out)
    return _launch("mg_nav_shape", dev, T, outs,
                   lambda: (dp, int(dpitch), P, N, W, H, ptr(pos_before), ptr(pos_after), ptr(age, torch.int32),
                            ptr(init_pos, torch.float32), ptr(done, torch.uint8), ptr(reward, torch.float32), T, float(scale),
                            float(gamma), SHAPE_ZERO_TERMINAL if zero_terminal else 0, ptr(outs[0], torch.float32),
                            ptr(outs[1], torch.float32), ptr(outs[2], torch.uint8)))


def goal_shape(type_plane, rec_t, rec_n, rec_goal, pos_before, pos_after, width, height, reward=None, done=None,
               pass_types=PASS_DEFAULT, age=None, init_pos=None, state=None, doors_open=False, scale=1.0, gamma=0.99,
               zero_terminal=False, out=None, shaping_out=None, mask_out=None):
    """shape for records that each name their own goal (mg_nav_goal_shape, include/minigrid_nav.h): the planes, the
    records (rec_t, rec_n int32[R], rec_goal float32[R, 2] = (y, x)), age and init_pos as goal_moves takes them,
    pos_before / pos_after float32[T, N, 2] as shape takes them; reward float32[R] (a record's own reward) or None, done
    uint8[R], required with zero_terminal=True.  -> (out float32[R], F float32[R], mask uint8[R]): per record what shape
    gives in the field of the record's env flooded from the record's goal cell; mask 0 (F = 0, the reward passed through)
    for a record whose t, n, goal or either position names nothing or has no path.  out / shaping_out / mask_out as in
    shape.  One launch (none for R = 0), no field in memory, no host synchronisation."""
    return _record_shape("mg_nav_goal_shape", None, type_plane, rec_t, rec_n, rec_goal, pos_before, pos_after, width, height,
                         reward, done, pass_types, age, init_pos, state, doors_open, scale, gamma, zero_terminal, out,
                         shaping_out, mask_out)


def timed_goal_shape(type_plane, rec_t, rec_n, rec_goal, pos_before, pos_after, width, height, blocked, age, init_pos,
                     reward=None, done=None, pass_types=PASS_DEFAULT, state=None, doors_open=False, scale=1.0, gamma=0.99,
                     zero_terminal=False, out=None, shaping_out=None, mask_out=None):
    """goal_shape for a world whose blockers move with a period (mg_nav_timed_goal_shape, include/minigrid_nav.h): the
    planes, the records, blocked, age (the clock as well) and init_pos (both required) as timed_goal_moves takes them;
    pos_before / pos_after float32[T, N, 2], reward float32[R] or None, done uint8[R] (required with zero_terminal=True),
    scale, gamma and the three outputs as goal_shape takes them.  -> (out float32[R], F float32[R], mask uint8[R]): per
    record what shape gives in the time-expanded field of the record's env flooded from the record's goal cell -- the
    acting cell at the phase of its age, the after cell at the phase that follows; mask 0 (F = 0, the reward passed
    through) for a record whose t, n, goal or either position names nothing, whose goal cell is free at no phase, or
    whose acting or after state is not free at its phase or has no path.  One launch (none for R = 0), no field in memory,
    no host synchronisation."""
    return _record_shape("mg_nav_timed_goal_shape", blocked, type_plane, rec_t, rec_n, rec_goal, pos_before, pos_after, width,
                         height, reward, done, pass_types, age, init_pos, state, doors_open, scale, gamma, zero_terminal, out,
                         shaping_out, mask_out)


def timed_goal_shape_floods(width, height, period):
    """How many of a workgroup's 8 half wavefronts flood at a time in timed_goal_shape at this size and period (8, 4, 2 or
    1: their images share 64 KiB of LDS with a staging larger than timed_goal_moves') -- the launch's own host function."""
    return query("mg_nav_timed_goal_shape_floods", int(width), int(height), int(period))


AHEAD_SIDE = 7                        # ahead: displacements -3..3 per axis, bit (dy + 3) * 7 + (dx + 3) of a label
AHEAD_MAX_STEPS = 3
AHEAD_DTYPE = torch.int64             # a uint64 label; bits 49..63 are 0, so the sign bit never is set


def ahead(field, pos, width, height, steps=3, age=None, init_pos=None, out=None, dist_out=None):
    """Where a shortest path leads in `steps` (1..3) steps from every acting state of a rollout (mg_nav_ahead,
    include/minigrid_nav.h, "Look-ahead").  field uint16[N, H*W] as distance_field returns it or uint16[N, P, H*W] as
    timed_field does (a 3-D field means timed, as in shape; rows may be padded); pos float32[T, N, 2] = (y, x) BEFORE each
    step, age int32[T, N] with init_pos float32[2] as optimal_moves takes them (required with a timed field: the age is
    the clock).  -> (labels int64[T, N], acting_dist uint16[T, N]): bit (dy + 3) * 7 + (dx + 3) of a label = some shortest
    path stands at displacement (dy, dx) after `steps` steps (at the goal it stays); 0 on an unreachable state or outside
    the world.  out / dist_out as in optimal_moves.  One launch (none for T = 0)."""
    W, H = int(width), int(height)
    dp, dpitch, N, P = _field_rows(field, W, H)
    dev = field.device
    T = _positions(N, dev, pos)
    _clock(age, init_pos, T, N, dev)
    assert age is not None or P == 1, "the age is the clock: age and init_pos are required with a timed field"
    out, dist_out = _moves_outputs((T, N), dev, AHEAD_DTYPE, out, dist_out)
    return _launch("mg_nav_ahead", dev, T, (out, dist_out),
                   lambda: (dp, int(dpitch), P, N, W, H, ptr(pos), ptr(age, torch.int32), ptr(init_pos, torch.float32), T,
                            int(steps), ptr(out, AHEAD_DTYPE), ptr(dist_out, DIST_DTYPE)))


def goal_ahead(type_plane, rec_t, rec_n, rec_goal, pos, width, height, steps=3, pass_types=PASS_DEFAULT, age=None,
               init_pos=None, state=None, doors_open=False, out=None, dist_out=None):
    """ahead for records that each name their own goal (mg_nav_goal_ahead, include/minigrid_nav.h): the planes, the
    records, pos, age and init_pos as goal_moves takes them.  -> (labels int64[R], acting_dist uint16[R]): per record what
    ahead gives in the field of the record's env flooded from the record's goal cell; 0 / UNREACHABLE for a record whose
    t, n, goal or acting position names nothing.  out / dist_out as in goal_moves.  One launch (none for R = 0), no field
    in memory, no host synchronisation."""
    return _record_ahead("mg_nav_goal_ahead", None, type_plane, rec_t, rec_n, rec_goal, pos, width, height, steps, pass_types,
                         age, init_pos, state, doors_open, out, dist_out)


def timed_goal_ahead(type_plane, rec_t, rec_n, rec_goal, pos, width, height, blocked, age, init_pos, steps=3,
                     pass_types=PASS_DEFAULT, state=None, doors_open=False, out=None, dist_out=None):
    """goal_ahead for a world whose blockers move with a period (mg_nav_timed_goal_ahead, include/minigrid_nav.h): the
    planes, the records, pos, blocked, age (the clock as well) and init_pos (both required) as timed_goal_moves takes them.
    -> (labels int64[R], acting_dist uint16[R]): per record what ahead gives in the time-expanded field of the record's env
    flooded from the record's goal cell, from the acting cell at the phase of its age -- the expert waits where the
    blockers make it; 0 / UNREACHABLE for a record whose t, n, goal or acting position names nothing, whose goal cell is
    free at no phase or whose state has no path.  out / dist_out as in goal_moves.  One launch (none for R = 0), no field
    in memory, no host synchronisation."""
    return _record_ahead("mg_nav_timed_goal_ahead", blocked, type_plane, rec_t, rec_n, rec_goal, pos, width, height, steps,
                         pass_types, age, init_pos, state, doors_open, out, dist_out)


def timed_goal_ahead_floods(width, height, period):
    """How many of a workgroup's 8 half wavefronts flood at a time in timed_goal_ahead at this size and period (8, 4, 2 or
    1: their images share 64 KiB of LDS with a staging larger than timed_goal_moves') -- the launch's own host function."""
    return query("mg_nav_timed_goal_ahead_floods", int(width), int(height), int(period))


def ahead_bits(labels):
    """Look-ahead labels int64[...] -> bool[..., 7, 7]: [..., i, j] = displacement (dy, dx) = (i - 3, j - 3) is in the
    label -- the classes of the orientation head's two 7-way distributions.  A torch op on any device."""
    assert labels.dtype == AHEAD_DTYPE
    sh = torch.arange(AHEAD_SIDE * AHEAD_SIDE, dtype=torch.int64, device=labels.device)
    return (((labels.unsqueeze(-1) >> sh) & 1) != 0).view(*labels.shape, AHEAD_SIDE, AHEAD_SIDE)


def ahead_loss(p0, p1, labels, coef, n_valid=None):
    """The set-valued prior of the orientation head, plain torch like the head's own NLL.  p0, p1 [B, 7]: the head's two
    distributions (any positive scale: they are normalised here), labels int64[B].  With q0, q1 the normalised
    probabilities, m[b] = sum_ij bits[b, i, j] * q0[b, i] * q1[b, j] is the mass the head puts on the label and
    l = -log(clamp(m, eps, 1 - eps)), eps = float32's;  term = coef * the mean of l over the rows below n_valid (None: all)
    with a non-zero label, 0 without such a row.  -> (term, stats): stats = {"rows": labelled rows, "mass": their summed m},
    detached 0-d tensors.  No host synchronisation."""
    B = labels.shape[0]
    assert p0.shape == (B, AHEAD_SIDE) and p1.shape == (B, AHEAD_SIDE)
    q0, q1 = p0 / p0.sum(-1, keepdim=True), p1 / p1.sum(-1, keepdim=True)
    bits = ahead_bits(labels).to(q0.dtype)
    m = ((bits * q1.unsqueeze(1)).sum(-1) * q0).sum(-1)
    eps = torch.finfo(torch.float32).eps
    lab = labels != 0
    if n_valid is not None:
        lab = lab & (torch.arange(B, device=labels.device) < int(n_valid))
    loss = -torch.log(m.clamp(eps, 1.0 - eps))
    rows_ = lab.sum()
    term = float(coef) * torch.where(lab, loss, torch.zeros_like(loss)).sum() / rows_.clamp(min=1).to(loss.dtype)
    return term, {"rows": rows_.detach(), "mass": torch.where(lab, m, torch.zeros_like(m)).sum().detach()}


PATH_SUMMARY = ("episodes", "successes", "rated", "spl_sum", "start_sum", "best_sum", "progress_sum", "off_sum",
                "steps_sum", "best_min")              # the ten entries of mg_nav_path_summary
_PATH_DTYPES = (DIST_DTYPE, DIST_DTYPE, torch.int32, torch.int32)       # start, best, off, steps


def _u16_zeros(shape, dev):
    """A zeroed uint16 tensor (torch's uint16 has views and copies, little else: made as int16)."""
    return torch.zeros(shape, dtype=torch.int16, device=dev).view(DIST_DTYPE)


def path_scan(field, pos_before, pos_after, width, height, terminated, truncated, carry, age=None, init_pos=None, out=None):
    """Path efficiency per episode, one step after the other (mg_nav_path_scan, include/minigrid_nav.h, "Path
    efficiency").  field uint16[N, H*W] as distance_field returns it or uint16[N, P, H*W] as timed_field does (rows may be
    padded); pos_before, pos_after float32[T, N, 2], age int32[T, N] and init_pos float32[2] as shape takes them (required
    with a timed field); terminated, truncated uint8[T, N]; carry = (start uint16[N], best uint16[N], off int32[N], steps
    int32[N]), updated in place -- all zero: no episode is running.  -> (ep_start uint16[T, N], ep_best uint16[T, N],
    ep_off int32[T, N], ep_steps int32[T, N]): at a done step the distance the ending episode started at, the least it
    stood at, its steps off a shortest path and its length.  out: a 4-tuple of tensors to write into, None = a new one,
    False = not wanted (None is returned for it); at least one is wanted.  One launch (none for T = 0)."""
    W, H = int(width), int(height)
    dp, dpitch, N, P = _field_rows(field, W, H)
    dev = field.device
    T = _positions(N, dev, pos_before, pos_after)
    _clock(age, init_pos, T, N, dev)
    assert age is not None or P == 1, "the age is the clock: age and init_pos are required with a timed field"
    for f in (terminated, truncated):
        assert f.shape == (T, N) and f.device == dev
    for c, dt in zip(carry, _PATH_DTYPES):
        assert c.shape == (N,) and c.device == dev and c.dtype == dt
    outs = []
    for o, dt in zip(out if out is not None else (None,) * 4, _PATH_DTYPES):
        o = torch.empty((T, N), dtype=dt, device=dev) if o is None else (None if o is False else o)
        assert o is None or (o.shape == (T, N) and o.device == dev and o.dtype == dt)
        outs.append(o)
    assert any(o is not None for o in outs), "no output wanted"
    return _launch("mg_nav_path_scan", dev, T, tuple(outs),
                   lambda: (dp, int(dpitch), P, N, W, H, ptr(pos_before), ptr(pos_after), ptr(age, torch.int32),
                            ptr(init_pos, torch.float32), ptr(terminated, torch.uint8), ptr(truncated, torch.uint8), T,
                            *(ptr(c) for c in carry), *(ptr(o) for o in outs)))


def path_summary_workspace(T, N):
    """Doubles of workspace path_summary needs for a [T, N] rollout -- the launch's own host function."""
    return query("mg_nav_path_summary_workspace", int(T), int(N))


def path_summary(ep_start, ep_best, ep_off, ep_steps, terminated, truncated, summary=None, workspace=None):
    """The episodes that ended in a rollout (mg_nav_path_summary): path_scan's four outputs and the flags, all [T, N] with
    T >= 1 -> summary float64[10] in the order of PATH_SUMMARY: episodes, successes, rated episodes (reachable start), the
    sums over the rated of SPL = success ? start / max(steps, start) : 0, of start, of best and of (start - best) / start,
    the sums of off and steps over all episodes, and the least best (+inf without a rated episode).  Deterministic: a
    fixed grid and order for a given (T, N).  summary / workspace: tensors to write into.  No host synchronisation."""
    T, N = terminated.shape
    dev = terminated.device
    for t, dt in zip((ep_start, ep_best, ep_off, ep_steps), _PATH_DTYPES):
        assert t.shape == (T, N) and t.device == dev and t.dtype == dt
    assert truncated.shape == (T, N) and truncated.device == dev
    if summary is None:
        summary = torch.empty(len(PATH_SUMMARY), dtype=torch.float64, device=dev)
    if workspace is None:
        workspace = torch.empty(path_summary_workspace(T, N), dtype=torch.float64, device=dev)
    assert summary.shape == (len(PATH_SUMMARY),) and workspace.numel() >= path_summary_workspace(T, N)
    call("mg_nav_path_summary", dev, ptr(ep_start), ptr(ep_best), ptr(ep_off), ptr(ep_steps), ptr(terminated, torch.uint8),
         ptr(truncated, torch.uint8), T, N, ptr(summary, torch.float64), ptr(workspace, torch.float64))
    return summary


class PathTracker:
    """Path efficiency of the episodes of N envs, carried across rollouts, in the style of EpisodeTracker / VisitTracker:
    account() per rollout (mg_nav_path_scan, mg_nav_path_summary: two calls, no host synchronisation), read() for the
    numbers of the last accounted rollout."""

    def __init__(self, num_envs, device, width, height, period=1):
        self.N, self.device = int(num_envs), torch.device(device)
        self.width, self.height, self.period = int(width), int(height), int(period)
        assert 1 <= self.period <= MAX_PERIOD
        d = self.device
        self.carry = (_u16_zeros(self.N, d), _u16_zeros(self.N, d), torch.zeros(self.N, dtype=torch.int32, device=d),
                      torch.zeros(self.N, dtype=torch.int32, device=d))         # start, best, off, steps
        self.summary = torch.zeros(len(PATH_SUMMARY), dtype=torch.float64, device=d)
        self.summary[-1] = float("inf")                                     # nothing accounted yet: no rated episode
        self.steps = self._workspace = None                                 # sized by the first account()

    def reset(self):
        """Forget the running episodes (envs were reset); the last summary stays."""
        for c in self.carry:
            c.view(torch.int16 if c.dtype == DIST_DTYPE else c.dtype).zero_()

    def account(self, field, pos_before, pos_after, terminated, truncated, age=None, init_pos=None):
        """Account one rollout: field uint16[N, H*W] (period 1) or uint16[N, P, H*W], the positions [T, N, 2] before and
        after each step, the flags [T, N], age [T, N] with init_pos (required with period > 1) as path_scan takes them.
        Afterwards `steps` = (ep_start, ep_best, ep_off, ep_steps) [T, N] hold the scan's outputs and `summary` the ten
        sums over the episodes that ended in this rollout."""
        T, N = terminated.shape
        assert N == self.N, "tracker made for %d envs, got %d" % (self.N, N)
        assert (field.shape[1] if field.dim() == 3 else 1) == self.period, "tracker made for period %d" % self.period
        if self.steps is None or self.steps[0].shape[0] != T:
            self.steps = tuple(torch.empty((T, N), dtype=dt, device=self.device) for dt in _PATH_DTYPES)
            self._workspace = torch.empty(path_summary_workspace(T, N), dtype=torch.float64, device=self.device)
        path_scan(field, pos_before, pos_after, self.width, self.height, terminated, truncated, self.carry, age=age,
                  init_pos=init_pos, out=self.steps)
        path_summary(*self.steps, terminated, truncated, summary=self.summary, workspace=self._workspace)

    def read(self):
        """The last account()'s summary as Python numbers (one device-to-host copy: the one sync): the entries of
        PATH_SUMMARY (best_min +inf without a rated episode) plus spl = spl_sum / rated, success_rate = successes /
        episodes, progress = progress_sum / rated and off_path_rate = off_sum / steps_sum, each None where its denominator
        is 0."""
        host = self.summary.cpu().tolist()
        out = dict(zip(PATH_SUMMARY, host))
        for k in ("episodes", "successes", "rated", "start_sum", "best_sum", "off_sum", "steps_sum"):
            out[k] = int(out[k])
        E, R, S = out["episodes"], out["rated"], out["steps_sum"]
        out["best_min"] = int(out["best_min"]) if R else float("inf")
        out["spl"] = out["spl_sum"] / R if R else None
        out["success_rate"] = out["successes"] / E if E else None
        out["progress"] = out["progress_sum"] / R if R else None
        out["off_path_rate"] = out["off_sum"] / S if S else None
        return out


TWOARMY_PERIOD = 6
_TWOARMY_BALL_X0 = (7, 8, 7, 6, 6, 6)      # x of the first of the three row-8 balls by step_move % 6 (twoarmy_v6.py:96-109)
_TWOARMY_V6_BLOCKS = ((4, 11), (5, 11), (4, 12), (5, 12), (8, 11), (8, 12), (9, 11), (9, 12))   # twoarmy_v6.py:186-197


def twoarmy_schedule(avoid_risk=False, blocks=False, device=None):
    """The period-6 schedule of Twoarmy's row-8 balls, int32[6, 17], built on the host: phase = step_move % 6, the balls
    at x0, x0 + 1, x0 + 2 of row 8 with x0 = 7, 8, 7, 6, 6, 6 (they move before the agent does, so phase p holds where
    they stand once step_move is p).  Use it with pass_types | PASS_BALL: the plane's own ball cells are then enterable
    and only the schedule blocks.  avoid_risk: also block, at the same phase, the row-9 cell under each ball (the -0.1
    cell of twoarmy_v6.py:241-243).  blocks: also block v6's two constant 2x2 wall blocks at every phase (they appear
    with the agent's first step out of the start corner).  device None: a host tensor."""
    rows = [[0] * 17 for _ in range(TWOARMY_PERIOD)]
    for p, x0 in enumerate(_TWOARMY_BALL_X0):
        rows[p][8] = 7 << x0
        if avoid_risk:
            rows[p][9] = 7 << x0
        if blocks:
            for x, y in _TWOARMY_V6_BLOCKS:
                rows[p][y] |= 1 << x
    return torch.tensor(rows, dtype=torch.int32, device=device)


def to_policy_mask(moves, n_actions):
    """Move sets (optimal_moves) as masks over POLICY indices, the inverse of the policy-index -> env-action map (policy
    index k < 4 is move k, the last index n_actions - 1 is the env's `done`): bits 0 .. min(4, n_actions - 1) - 1 stay, the
    stay bit moves to bit n_actions - 1.  A torch op on uint8 tensors of any shape."""
    A = int(n_actions)
    assert moves.dtype == torch.uint8 and 2 <= A <= 8
    low = moves & ((1 << min(4, A - 1)) - 1)
    return low | (((moves >> 4) & 1) << (A - 1))


def as_int(t):
    """uint16 distances as int32 (whatever 16-bit dtype stores them)."""
    return t.view(torch.int16).to(torch.int32) & 0xFFFF
