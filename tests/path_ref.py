"""Numpy restatement of the path-efficiency routines of include/minigrid_nav.h ("Path efficiency"; mg_nav_path_scan,
mg_nav_path_summary): one env and one step at a time, in step order, the sums sequential and in float64.  The two distances
of a step are the ones the shaping restatement reads (shape_ref.distances, on the fields of nav_ref.py / timed_nav_ref.py).
The reference project has no counterpart: this restatement is the oracle.  Test-side only."""
import numpy as np

import nav_ref
import shape_ref

UNREACHABLE = nav_ref.UNREACHABLE
SUMMARY = ("episodes", "successes", "rated", "spl_sum", "start_sum", "best_sum", "progress_sum", "off_sum", "steps_sum",
           "best_min")


def zero_carry(N):
    """(start uint16[N], best uint16[N], off int32[N], steps int32[N]), all zero: no episode is running."""
    return np.zeros(N, np.uint16), np.zeros(N, np.uint16), np.zeros(N, np.int32), np.zeros(N, np.int32)


def on_path(d_before, d_after):
    return d_before != UNREACHABLE and d_before >= 1 and d_after == d_before - 1


def scan_distances(d_before, d_after, terminated, truncated, carry):
    """The scan on the two distances of every step, integer[T, N] -> ((ep_start uint16, ep_best uint16, ep_off int32,
    ep_steps int32)[T, N], the carries afterwards).  `carry` is not modified."""
    T, N = np.asarray(terminated).shape
    start, best, off, steps = (np.array(c).copy() for c in carry)
    out = (np.zeros((T, N), np.uint16), np.zeros((T, N), np.uint16), np.zeros((T, N), np.int32), np.zeros((T, N), np.int32))
    for n in range(N):
        s, b, o, k = int(start[n]), int(best[n]), int(off[n]), int(steps[n])
        for t in range(T):
            db, da = int(d_before[t, n]), int(d_after[t, n])
            if k == 0:
                s = b = db
                o = 0
            k += 1
            if not on_path(db, da):
                o += 1
            b = min(b, da)
            out[0][t, n], out[1][t, n], out[2][t, n], out[3][t, n] = s, b, o, k
            if terminated[t, n] or truncated[t, n]:
                k = 0
        start[n], best[n], off[n], steps[n] = s, b, o, k
    return out, (start, best, off, steps)


def path_scan(dist, pos_before, pos_after, W, H, terminated, truncated, carry, age=None, init_pos=None):
    """mg_nav_path_scan: dist uint16[N, H*W] or [N, P, H*W] -> (the four outputs, the carries afterwards)."""
    db, da = shape_ref.distances(dist, pos_before, pos_after, W, H, age, init_pos)
    return scan_distances(db, da, terminated, truncated, carry)


def path_summary(ep_start, ep_best, ep_off, ep_steps, terminated, truncated):
    """mg_nav_path_summary -> float64[10] in the order of SUMMARY, the done steps folded in row-major order."""
    v = np.zeros(10, np.float64)
    v[9] = np.inf
    ts, ns = np.nonzero((np.asarray(terminated) != 0) | (np.asarray(truncated) != 0))      # row-major order
    for t, n in zip(ts.tolist(), ns.tolist()):
        s, b, o, k = int(ep_start[t, n]), int(ep_best[t, n]), int(ep_off[t, n]), int(ep_steps[t, n])
        v[0] += 1
        v[1] += 1 if terminated[t, n] else 0
        v[7] += o
        v[8] += k
        if s == UNREACHABLE:
            continue
        v[2] += 1
        if terminated[t, n]:
            v[3] += np.float64(s) / np.float64(max(k, s))
        v[4] += s
        v[5] += b
        if s >= 1:
            v[6] += np.float64(s - b) / np.float64(s)
        v[9] = min(v[9], b)
    return v


def derived(v):
    """What PathTracker.read() derives from the ten entries; None where a denominator is 0."""
    E, R, S = v[0], v[2], v[8]
    return {"spl": v[3] / R if R else None, "success_rate": v[1] / E if E else None,
            "progress": v[6] / R if R else None, "off_path_rate": v[7] / S if S else None}
