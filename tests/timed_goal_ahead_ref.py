"""Host restatement of mg_nav_timed_goal_ahead (include/minigrid_nav.h), made by composition: per record the queue BFS over
(cell, phase) of the record's env from the record's goal cell (timed_nav_ref.field), then the frontier loop of ahead_ref.label
from the acting cell at the phase of the record's clock.  The only thing shared between records is a memo of (env, goal
cell) -> field; the order of the records is immaterial.  Below it: the three worlds the CPU and the GPU test share, numpy
only (the Twoarmy planes come from the oracle's reset).  Test-side only."""
import numpy as np

import ahead_ref
import nav_ref
import timed_nav_ref as tref
import visit_ref

UNREACHABLE = tref.UNREACHABLE
BALL = 1 << 6
STATIC = nav_ref.PASS_DEFAULT | BALL                                  # balls enterable: only the schedule blocks
STAY = 24
KINDS = ("t", "n", "goal_no_cell", "goal_never_free", "acting_no_cell", "unreachable")


def goal_field(c, n, gc, memo=None):
    """uint16[P, H*W] of env n of the world c flooded from the goal cell gc, kept in the world's memo."""
    memo = c["memo"] if memo is None else memo
    if (n, gc) not in memo:
        W, H = c["W"], c["H"]
        sched = c["sched"] if c["sched"].ndim == 2 else c["sched"][n]
        memo[(n, gc)] = tref.field(c["ty"][n], None if c["st"] is None else c["st"][n], W, H, sched, c["P"], c["pass_types"],
                                   goal=(gc % W, gc // W))["dist"]
    return memo[(n, gc)]


def kind_of(c, rec_t, rec_n, rec_goal, b):
    """The bad-record rule, written out once: the first reason for which record b names nothing, or (None, field, acting
    cell, phase) for a record with a state to label."""
    W, H, N, T = c["W"], c["H"], c["N"], c["T"]
    t, n = int(rec_t[b]), int(rec_n[b])
    if not 0 <= t < T:
        return "t", None, None, None
    if not 0 <= n < N:
        return "n", None, None, None
    gc = visit_ref.cell_of(rec_goal[b][0], rec_goal[b][1], W, H)
    if gc >= W * H:
        return "goal_no_cell", None, None, None
    field = goal_field(c, n, gc)
    if (field[:, gc] == UNREACHABLE).all():
        return "goal_never_free", None, None, None
    clock = int(c["age"][t, n])
    q = c["init"] if clock <= 0 else c["pos"][t, n]
    ac = visit_ref.cell_of(q[0], q[1], W, H)
    if ac >= W * H:
        return "acting_no_cell", None, None, None
    ph = tref.phase_of(clock, c["P"])
    if field[ph, ac] == UNREACHABLE:
        return "unreachable", None, None, None
    return None, field, ac, ph


def timed_goal_ahead(c, rec_t, rec_n, rec_goal, steps):
    """-> (labels uint64[R], acting_dist uint16[R]) of the records on the world c (its planes, schedule, rollout)."""
    R = len(rec_t)
    lab, ad = np.zeros(R, np.uint64), np.full(R, UNREACHABLE, np.uint16)
    for b in range(R):
        kind, field, ac, ph = kind_of(c, rec_t, rec_n, rec_goal, b)
        if kind is None:
            lab[b], ad[b] = ahead_ref.label(field, c["W"], c["H"], ac, ph, steps)
    return lab, ad


def kinds(c, rec):
    return [kind_of(c, rec["t"], rec["n"], rec["goal"], b)[0] for b in range(len(rec["t"]))]


# ------------------------------------------------------------------------------------------------ the worlds of both tests
_WORLDS = {}


def _walk(rng, free, W, H, T, N, start, stray=0.05):
    """A seeded walk per env over the cells of `free` (bool[N, H, W]): a move or a wait per step, a move into a cell that
    is not free is not made; with probability `stray` the position is anywhere, walls and the outside included."""
    pos = np.zeros((T, N, 2), np.float32)
    xy = np.array(start)
    for t in range(T):
        for n in range(N):
            dx, dy = ((-1, 0), (1, 0), (0, -1), (0, 1), (0, 0))[rng.integers(0, 5)]
            x, y = xy[n, 0] + dx, xy[n, 1] + dy
            if 0 <= x < W and 0 <= y < H and free[n, y, x]:
                xy[n] = (x, y)
            pos[t, n] = (xy[n, 1], xy[n, 0])
            if rng.random() < stray:
                pos[t, n] = (rng.integers(-1, H + 1), rng.integers(-1, W + 1))
        pos[t] += rng.choice([0.0, 0.5, 0.999], (N, 2)).astype(np.float32)
    return pos


def _clocks(rng, T, N, P):
    """Ages that run on with the steps from a start far beyond P, back to 0 at a reset now and then; one below 0."""
    age = np.zeros((T, N), np.int32)
    a = rng.integers(1, 5 * P + 3, N)
    for t in range(T):
        a = np.where(rng.random(N) < 0.06, 0, a)
        age[t] = a
        a = a + 1
    age[T // 2, 0] = -2
    return age


def _off_cells(c, never_free, bad_pos, on_it):
    """Two positions of the rollout for _plant: bad_pos = (t, n) is no cell, on_it = (t, n) stands on the cell `never_free`."""
    for (t, n), q in ((bad_pos, (np.nan, 0.5)), (on_it, (never_free // c["W"] + 0.5, never_free % c["W"] + 0.5))):
        c["age"][t, n] = 7 + t                                        # the position is read, not init_pos
        c["pos"][t, n] = q


def _walk_cell(c, t, n):
    """The cell of the walk of env n at step t, a stray position clipped into the world."""
    y, x = np.clip(np.floor(c["pos"][t, n]), 0, (c["H"] - 1, c["W"] - 1)).astype(int)
    return int(y * c["W"] + x)


def _plant(rec, c, never_free, bad_pos, on_it):
    """The records that name nothing, from record 3 on: rec_t and rec_n out of range, three goals that are no cell, a goal
    that is free at no phase; bad_pos = (t, n) of a position that is no cell, on_it = (t, n) of one on a cell that is never
    free (an unreachable state)."""
    W, H, N, T = c["W"], c["H"], c["N"], c["T"]
    t, n, goal = rec["t"], rec["n"], rec["goal"]
    t[3], t[5] = -1, T
    n[7], n[9] = -1, N
    t[-1] = n[-1] = 0x7FFFFFFF
    t[-2] = n[-2] = -0x80000000
    goal[11], goal[12], goal[13] = (np.nan, 1.0), (H, 0.5), (0.5, -0.25)
    goal[15] = (never_free // W + 0.5, never_free % W + 0.25)
    t[17], n[17] = bad_pos
    g = c["pool"][bad_pos[1]][0]                                      # a goal of that env's own pool
    goal[17] = (g // W + 0.5, g % W + 0.5)
    t[19], n[19] = on_it
    g = c["pool"][on_it[1]][0]
    goal[19] = (g // W + 0.5, g % W + 0.5)
    return rec


def _records_of_runs(rng, c, R, max_run):
    """R records as ppo_her_relabel emits them: runs of consecutive steps of one env under one goal of its pool."""
    W, T = c["W"], c["T"]
    t, n, g = [], [], []
    while len(t) < R:
        L = int(min(R - len(t), 1 + rng.integers(0, max_run)))
        e = int(rng.integers(0, c["N"]))
        t0 = int(rng.integers(0, T))
        t += [(t0 + k) % T for k in range(L)]
        n += [e] * L
        g += [int(c["pool"][e][rng.integers(0, len(c["pool"][e]))])] * L
    g = np.array(g)
    goal = (np.stack([g // W, g % W], 1) + rng.choice([0.0, 0.25, 0.999], (R, 2))).astype(np.float32)
    return dict(t=np.array(t, np.int32), n=np.array(n, np.int32), goal=goal)


def _finish(c, rec):
    for a in (c["ty"], c["sched"], c["pos"], c["age"], c["init"]) + tuple(rec.values()):
        a.setflags(write=False)
    c["rec"], c["memo"], c["want"] = rec, {}, {}
    return c


def want(c, steps):
    """The reference outputs of the world's own records, computed once per steps and shared."""
    if steps not in c["want"]:
        c["want"][steps] = timed_goal_ahead(c, c["rec"]["t"], c["rec"]["n"], c["rec"]["goal"], steps)
    return c["want"][steps]


def small(P):
    """5 x 4 (the smallest world in which a frontier of radius 3 meets a border), random walls and types, a random schedule
    per env, 3 envs, T = 8, R = 70."""
    key = ("small", P)
    if key in _WORLDS:
        return _WORLDS[key]
    W, H, N, T, R = 5, 4, 3, 8, 70
    rng = np.random.default_rng(540 + P)
    ty, st = np.zeros((N, W * H), np.uint8), np.zeros((N, W * H), np.uint8)
    for n in range(N):
        ty[n], st[n] = nav_ref.random_world(rng, W, H, (0.1, 0.2)[n % 2], all_types=False)
    ty[0, 3 * W + 4] = 2                                              # a wall for the goal that is free at no phase
    sched = np.stack([tref.random_schedule(rng, P, H, 0.1 if P > 1 else 0.03) for _ in range(N)])
    free = np.stack([nav_ref.open_cells(ty[n], st[n], W, H) for n in range(N)])
    c = dict(W=W, H=H, N=N, T=T, P=P, ty=ty, st=st, sched=sched, pass_types=nav_ref.PASS_DEFAULT,
             init=np.array([H - 0.5, 0.25], np.float32))
    c["pos"] = _walk(rng, free, W, H, T, N, [np.argwhere(free[n])[0][::-1] for n in range(N)], stray=0.1)
    c["age"] = _clocks(rng, T, N, P)
    _off_cells(c, 3 * W + 4, (2, 1), (5, 0))
    # goals at the far end of the walks (which start at the first free cell), so that three steps do not reach them
    cells = [np.flatnonzero(free[n].reshape(-1)) for n in range(N)]
    c["pool"] = [[int(cells[n][-1]), int(cells[n][-2]), _walk_cell(c, T // 2, n)] for n in range(N)]
    import nav_util
    t, n, goal = nav_util.random_records(rng, c, R, T, mean_run=4)
    rec = _plant(dict(t=t, n=n, goal=goal), c, 3 * W + 4, (2, 1), (5, 0))
    rec["n"][15] = 0
    return _WORLDS.setdefault(key, _finish(c, rec))


def twoarmy():
    """17 x 17: the planes of Twoarmy v6 at a reset under the period-6 schedule of its balls and blocks, 4 envs, T = 50, walks
    that start under the door gap, R = 2100 records in runs: three workgroups, a run across either boundary."""
    if "twoarmy" in _WORLDS:
        return _WORLDS["twoarmy"]
    import twoarmy_oracle as orc
    from twoarmy_amd import minigrid_nav
    W = H = 17
    N, T, P, R = 4, 50, 6, 2100
    rng = np.random.default_rng(1706)
    ty = np.tile(np.frombuffer(orc.OracleEnv(6).e.type, np.uint8).copy()[None], (N, 1))
    sched = minigrid_nav.twoarmy_schedule(blocks=True).numpy().astype(np.uint32)
    free = np.stack([nav_ref.open_cells(ty[n], None, W, H, STATIC) for n in range(N)])
    c = dict(W=W, H=H, N=N, T=T, P=P, ty=ty, st=None, sched=sched, pass_types=STATIC, init=np.array([15.5, 1.5], np.float32))
    c["pos"] = _walk(rng, free, W, H, T, N, [(6 + 2 * n, 9 + n % 2) for n in range(N)])
    c["age"] = _clocks(rng, T, N, P)
    block = 11 * W + 4                                                # a cell of v6's wall blocks: scheduled at every phase
    _off_cells(c, block, (9, 2), (20, 1))
    # goals beyond the gap, in the gap (under a ball in some phases), and anywhere
    c["pool"] = [[6 * W + 8, 8 * W + 7 + n % 3, 4 * W + 3 + n, int(rng.choice(np.flatnonzero(free[n].reshape(-1))))]
                 for n in range(N)]
    rec = _records_of_runs(rng, c, R, 40)
    rec = _plant(rec, c, block, (9, 2), (20, 1))
    return _WORLDS.setdefault("twoarmy", _finish(c, rec))


def large():
    """32 x 32, an open room with a few walls, a random schedule per env at P = 16 (one flood at a time), 2 envs, R = 40."""
    if "large" in _WORLDS:
        return _WORLDS["large"]
    W = H = 32
    N, T, P, R = 2, 12, 16, 40
    rng = np.random.default_rng(3216)
    ty = np.where(rng.random((N, W * H)) < 0.04, 2, 1).astype(np.uint8)
    ty[:, 20 * W + 20] = 2
    sched = np.stack([tref.random_schedule(rng, P, H, 0.08) for _ in range(N)])
    free = np.stack([nav_ref.open_cells(ty[n], None, W, H) for n in range(N)])
    c = dict(W=W, H=H, N=N, T=T, P=P, ty=ty, st=None, sched=sched, pass_types=nav_ref.PASS_DEFAULT,
             init=np.array([30.5, 1.25], np.float32))
    c["pos"] = _walk(rng, free, W, H, T, N, [(29, 2), (3, 30)])
    c["age"] = _clocks(rng, T, N, P)
    _off_cells(c, 20 * W + 20, (4, 1), (7, 0))
    c["pool"] = [[_walk_cell(c, T // 2, n), int(rng.choice(np.flatnonzero(free[n].reshape(-1)))), 0 if free[n, 0, 0] else 1] for n in range(N)]
    rec = _plant(_records_of_runs(rng, c, R, 5), c, 20 * W + 20, (4, 1), (7, 0))
    return _WORLDS.setdefault("large", _finish(c, rec))


def worlds():
    """name -> world, every world of the GPU test."""
    return {"5x4 P=1": small(1), "5x4 P=2": small(2), "5x4 P=16": small(16), "17x17 Twoarmy": twoarmy(), "32x32 P=16": large()}
