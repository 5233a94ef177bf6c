"""float64 statement of ppo_gae_runs and a numpy restatement of ppo_run_ends (include/twoarmy_ppo.h), shared by
test_gae_runs_cpu.py, test_gae_runs_gpu.py and the two cases of test_streams_gpu.py, with the record generator and the
rounding bound of the scan they use.  A plain module like update_stats_ref.py; it mirrors _gae64 of
test_ppo_kernels_edges_gpu.py, along a flat record array cut at the run ends instead of along the columns of a tile.

The exact families (exact_inputs, exact_runs, boundary_runs) serve the boundary sweep of the scan tree, where a rounding
bound that grows with the run length would pass a wrong carry.  Their inputs make float32 arithmetic exact, so every
association order -- the shuffle scan, the folds across chunks and wavefronts, the carries between the levels -- gives
one answer and the kernel is compared bit for bit.  Why they are exact: every combine of the kernels keeps the c != 0
guard, so a composite never reaches past a run end or a masked done; whatever value the kernel forms, in a register, in
the workspace or in an output, is therefore prod(c) * (a sum of c-weighted deltas) over a CONTIGUOUS PIECE OF ONE RUN.
  c = 1 (gamma = lambda = 1): the deltas are integers, a piece's value is a partial sum of them, and assert_exact bounds
      the largest |partial sum| over every contiguous piece of every run (max minus min of the run's prefix sums) below
      2^24: integers below 2^24 add exactly.  exact_inputs telescopes the deltas (w[j] - w[j + 1], w in [0, 1000]), so
      the bound holds for runs of any length.
  c = 1/2 (gamma = 1/2, lambda = 1 and the converse): integer deltas |d| <= 15 in runs of L <= 16 records.  Every product
      of c is a power of two >= 2^-(L-1); a piece's value is a multiple of 2^-(L-1) of magnitude < 2 max|d| (+ max|v|
      for ret): (L - 1) + 5 = 20 bits of the 24.  assert_exact checks that budget from the data.
The deltas are split over reward, next_value and value as small integers, so the kernel's three-step delta
(gamma * nv, + r, - v) works on all three arrays, each step exact."""
import numpy as np

EPS32 = 2.0 ** -23
CHUNK, WAVE, BLOCK = 64, 512, 2048               # records per shuffle scan / per wavefront (GR_WAVE) / per workgroup (GR_BLOCK)
# The structural edges of the scan tree, in records.  Level 0 are the records, level 1 the composites of level 0's
# workgroups (one map per 2048 records), level 2 those of level 1: H <= 2048 is one launch, H <= 2048^2 three, beyond five.
LEVEL_EDGES = ((CHUNK, WAVE, BLOCK), (CHUNK * BLOCK, WAVE * BLOCK, BLOCK * BLOCK))
EDGES = LEVEL_EDGES[0] + LEVEL_EDGES[1]
EDGE_NAMES = dict(zip(EDGES, ("chunk0", "wave0", "block0", "chunk1", "wave1", "block1")))


def run_ends(t, n, goal, done):
    """(run_end uint8[H], broken): run_end_j = 0 iff record j is not done and record j + 1 is the next step of the same
    env under the same goal (float compares: NaN never links, -0.0 == +0.0); broken = records that are not done and
    still end a run."""
    t, n, goal, done = np.asarray(t, np.int64), np.asarray(n), np.asarray(goal), np.asarray(done)
    H = len(t)
    link = np.zeros(H, bool)
    link[:-1] = (done[:-1] == 0) & (n[1:] == n[:-1]) & (t[1:] == t[:-1] + 1) & (goal[1:, 0] == goal[:-1, 0]) & \
        (goal[1:, 1] == goal[:-1, 1])
    return (~link).astype(np.uint8), int(((done == 0) & ~link).sum())


def gae_runs64(r, v, nv, done, run_end, gamma, lam, use_mask):
    """The formula in float64 on the float32 inputs, parameters as the kernel sees them: fp32(gamma) and
    c = fp32(fp32(gamma) * fp32(lambda)) * cut, c = 0 at a run end and at the last record.  Where c = 0, A_j = delta_j
    exactly (nothing behind enters).  Returns adv, target, ret, the magnitude sum
    S_j = sum over k >= j of the same run of prod(c) * (|r_k| + |gamma nv_k| + |v_k|), and L_j = the number of records
    k >= j that enter A_j (1 where c_j = 0)."""
    g32 = np.float32(gamma)
    c32 = float(np.float32(g32 * np.float32(lam)))
    H = len(r)
    cut = (1.0 - (np.asarray(done) != 0)) if use_mask else np.ones(H)
    r, v, nv = (np.asarray(x, np.float32).astype(np.float64) for x in (r, v, nv))
    tgt = r + float(g32) * nv * cut
    delta = tgt - v
    mag = np.abs(r) + np.abs(float(g32) * nv) + np.abs(v)
    c = c32 * cut
    c[np.asarray(run_end) != 0] = 0.0
    c[H - 1] = 0.0
    adv, S, L = np.zeros(H), np.zeros(H), np.ones(H, np.int64)
    nxt, snx, lnx = 0.0, 0.0, 0
    cl, dl, ml = c.tolist(), delta.tolist(), mag.tolist()
    for j in range(H - 1, -1, -1):
        if cl[j] != 0.0:
            nxt, snx, lnx = dl[j] + cl[j] * nxt, ml[j] + cl[j] * snx, lnx + 1
        else:
            nxt, snx, lnx = dl[j], ml[j], 1
        adv[j], S[j], L[j] = nxt, snx, lnx
    return adv, tgt, adv + v, S, L


def one_step32(r, v, nv, done, gamma, use_mask):
    """The one-step formula in float32 with the reference's rounding order (PPO.py:113-114): target, delta."""
    r, v, nv = (np.asarray(x, np.float32) for x in (r, v, nv))
    cut = (1 - (np.asarray(done) != 0)).astype(np.float32) if use_mask else np.ones(len(r), np.float32)
    t32 = r + (np.float32(gamma) * nv) * cut
    return t32, t32 - v


def inputs(H, seed):
    rs = np.random.RandomState(seed)
    r, v, nv = (rs.randn(H).astype(np.float32) for _ in range(3))
    return r, v, nv


def pattern(kind, H, seed=0):
    """run_end uint8[H] of a run pattern: "singletons"; "runs64" / "runs64+1": runs of exactly 64 from index 0 / 1;
    "her": random lengths 1..64; "her16": random lengths 1..16; "one1000": one run of 1000 amid random short ones
    (H >= 3000); "whole": one run."""
    e = np.zeros(H, np.uint8)
    if kind == "singletons":
        e[:] = 1
    elif kind in ("runs64", "runs64+1"):
        first = 0 if kind == "runs64" else 1
        e[first + 63::64] = 1
        if first:
            e[0] = 1
    elif kind in ("her", "her16", "one1000"):
        rs = np.random.RandomState(1000 + seed)
        ends = np.cumsum(rs.randint(1, 17 if kind == "her16" else 65, H)) - 1
        e[ends[ends < H]] = 1
        if kind == "one1000":
            assert H >= 3000
            a = BLOCK - 300                                    # starts in one 2048-record workgroup, ends in the next
            e[a - 1] = 1
            e[a:a + 1000] = 0
            e[a + 999] = 1
    else:
        assert kind == "whole"
    e[H - 1] = 1
    return e


def dones(run_end, seed, mid_run=0.02):
    """Done flags in the shape of hindsight records: every run end is done, plus a few done records inside runs (which
    the done mask cuts at and reference mode scans through)."""
    rs = np.random.RandomState(2000 + seed)
    return (run_end | (rs.rand(len(run_end)) < mid_run)).astype(np.uint8)


def _records(H, seed):
    """Records in ppo_her_relabel's shape: runs of 1..64 consecutive steps of one env under one goal, each ending done."""
    rs = np.random.RandomState(seed)
    end = pattern("her", H, seed)
    run = np.concatenate([[0], np.cumsum(end)[:-1]]).astype(np.int64)          # run index of every record
    start = np.concatenate([[0], np.nonzero(end)[0] + 1])[run]
    t = (rs.randint(0, 50, run.max() + 1)[run] + np.arange(H) - start).astype(np.int32)
    n = rs.randint(0, 64, run.max() + 1)[run].astype(np.int32)
    goal = rs.randint(0, 17, (run.max() + 1, 2))[run].astype(np.float32)
    done = end.copy()
    done[H - 1] = rs.randint(0, 2)                                 # the array may stop in mid-run
    return t, n, goal, done


def _levels(H):
    levels, n = 1, H
    while n > BLOCK:
        n, levels = -(-n // BLOCK), levels + 1
    return levels


def _k(L, H):
    """k of |adv - adv64| <= k * EPS32 * S_j, counted in roundings of 2^-24 = EPS32 / 2 (each relative to a partial
    magnitude <= S_j) along the longest path of one term delta_k, k >= j, into A_j; L_j terms enter A_j.

    Every term: 3 roundings of delta (gamma * nv, + r, - v).  Its coefficient is a product of k - j <= L_j - 1 factors c,
    joined pairwise by the shuffle scan, the folds and the carries: at most L_j - 2 multiplications (any order of
    evaluation, a serial one too, rounds a product of m factors m - 1 times).

    L_j <= 64: the terms lie in the chunk of j and the next one.  The partial sum a term sits in is rounded by the <= 6
    fmas of the shuffle scan of its own chunk, by the fma that takes the value into the chunk (gr_eval), and, if it comes
    from the next chunk, by the fma of gr_eval in the chunk of j: <= 8.  The run ends inside that next chunk, so its
    composite has c = 0, and whatever lies between the two chunks -- a wavefront's fold, a workgroup's composite, the
    levels above -- hands (0, d) on through the c == 0 branches without arithmetic.  3 + 62 + 8 = 73, one more for the
    second-order terms of (1 + 2^-24)^73: k = 74 / 2 = 37, whatever H and wherever the run lies.

    Longer runs: the sum a term sits in is rounded, per level of the tree it visits, by <= 6 shuffle fmas + 8 chunk folds
    + 4 wavefront folds on the way up and <= 3 wavefronts + 8 chunks + 1 on the way down: 31.  A run inside one
    workgroup visits level 0 only; a run that crosses a workgroup carry visits at most every level H has.  So
    2 k = 3 + (L_j - 1) + 31 * levels visited + 1.  The run length enters because the coefficient of the farthest term is
    a product of L_j - 1 factors; a run that crosses w carries has L_j <= 2048 (w + 1)."""
    j = np.arange(len(L))
    crosses = (j // BLOCK) != ((j + L - 1) // BLOCK)
    visited = np.where(crosses, _levels(H), 1)
    return np.where(L <= CHUNK, 37.0, (L + 3 + 31 * visited) / 2.0)


# ------------------------------------------------------------------------------------------------ the exact families
FAMILIES = {"c1": (1.0, 1.0), "half_gamma": (0.5, 1.0), "half_lambda": (1.0, 0.5)}     # name -> (gamma, lambda)
VARIANTS = ("ends", "straddle", "long")          # the three placements of a run around an edge; "long" for c = 1 only


def variants(family):
    return VARIANTS if family == "c1" else VARIANTS[:2]


def boundaries(H):
    """The structural edges below H: record B exists and begins a new chunk / wavefront / workgroup of its level."""
    return [B for B in EDGES if B < H]


def exact_inputs(family, H, seed):
    """(reward, value, next_value) float32, small integers.  c1: delta_j = w[j] - w[j + 1] without the mask, w integers
    in [0, 1000], so a contiguous partial sum is w[a] - w[b]; the halves: delta in [-9, 9].  gamma * nv in [-8, 8] /
    [-3, 3] (what the mask takes out of delta at a done record: |delta| stays <= 12 for the halves), value likewise."""
    gamma, _ = FAMILIES[family]
    rs = np.random.RandomState(3000 + seed)
    if family == "c1":
        w = rs.randint(0, 1001, H + 1)
        delta, gnv, v = w[:-1] - w[1:], rs.randint(-8, 9, H), rs.randint(-8, 9, H)
    else:
        delta, gnv, v = rs.randint(-9, 10, H), rs.randint(-3, 4, H), rs.randint(-3, 4, H)
    nv = gnv * int(round(1.0 / gamma))                               # gamma = 1/2: even next values
    return tuple(x.astype(np.float32) for x in (delta - gnv + v, v, nv))


def boundary_runs(H, bounds, variant, short, seed=0):
    """(run_end uint8[H], placed): "her" runs (short: runs of <= 16) and on top of them, around EVERY edge B of `bounds`,
    the run of this variant; placed = [(first, last)] of the runs put on top, which never overlap.
      "ends":     one run ends on record B - 1 and the next begins exactly on B (4 records each);
      "straddle": one run from B - 3 to B + 2;
      "long":     one run that starts well before B and ends well after it, two whole units of the next smaller edge on
                  either side (2 * 2048 records around a level-1 chunk edge, 2 * 64 * 2048 around a level-1 wavefront
                  edge); across the level-2 edge at 2048^2 from five workgroups before it to the last record; and, once H
                  reaches 2048^2, one run over the whole third wavefront of level 1 (records 2 * 2^20 .. 3 * 2^20) and
                  three workgroups beyond it on either side, the only place where a fold across level 1's wavefronts
                  meets a c != 0.
    Runs are clipped to the array."""
    assert variant in VARIANTS and all(0 < B < H for B in bounds)
    e = pattern("her16" if short else "her", H, seed)
    placed = []

    def put(a, b):
        a, b = max(a, 0), min(b, H - 1)
        if a > 0:
            e[a - 1] = 1
        e[a:b] = 0
        e[b] = 1
        placed.append((a, b))

    for B in bounds:
        if variant == "ends":
            put(B - 4, B - 1)
            put(B, B + 3)
        elif variant == "straddle":
            put(B - 3, B + 2)
        elif B == BLOCK * BLOCK:
            put(B - 5 * BLOCK, H - 1)
        else:
            unit = max([x for x in EDGES if x < B], default=12)
            put(B - 2 * unit, B + 2 * unit - 1)
    if variant == "long" and H >= BLOCK * BLOCK:
        put(2 * WAVE * BLOCK - 3 * BLOCK, 3 * WAVE * BLOCK + 3 * BLOCK - 1)
    placed.sort()
    assert all(x[1] < y[0] for x, y in zip(placed, placed[1:])), placed
    assert not short or np.diff(np.concatenate([[-1], np.nonzero(e)[0]])).max() <= 16
    return e, placed


def boundary_dones(run_end, bounds, variant, seed):
    """dones(): every run end and 2 % of the other records; and a done record beside every edge, inside a run where the
    array allows: record B - 1 in the run that straddles B, record B in the run that begins on B and in the long run."""
    d = dones(run_end, seed)
    for B in bounds:
        d[B - 1 if variant == "straddle" else B] = 1
    return d


def _run_extrema(P0, start, op):
    """op over P0[s .. e + 1] for every run [s, e]: the prefix before its first record and after each of its records."""
    return op(op.reduceat(P0[:-1], start), op.reduceat(P0[1:], start))


def assert_exact(delta, v, run_end, c):
    """The condition of the exact families (module docstring), asserted on the host before anything is launched; inputs
    that break it are a bug of the test that made them."""
    H = len(delta)
    assert c in (1.0, 0.5) and (delta == np.rint(delta)).all() and (v == np.rint(v)).all()
    end = np.asarray(run_end) != 0
    end[H - 1] = True
    start = np.concatenate([[0], np.nonzero(end)[0][:-1] + 1])
    if c == 1.0:
        P0 = np.concatenate([[0], np.cumsum(delta.astype(np.int64))])
        spread = int((_run_extrema(P0, start, np.maximum) - _run_extrema(P0, start, np.minimum)).max())
        assert spread + int(np.abs(v).max()) < 2 ** 24, "a partial sum of %d does not fit float32" % spread
    else:
        longest = int(np.diff(np.concatenate([start, [H]])).max())
        magnitude = 2 * int(np.abs(delta).max()) + int(np.abs(v).max())      # |A| < 2 max|d|, |ret| <= |A| + |v|
        bits = (longest - 1) + max(magnitude, 1).bit_length()
        assert bits <= 24, "runs of %d records and magnitudes of %d need %d bits" % (longest, magnitude, bits)


def exact_runs(r, v, nv, done, run_end, gamma, lam, use_mask):
    """gae_runs64 for the exact families, vectorised: (adv, target, ret) in float64, every value a float32.  c = 1: the
    suffix sums of each piece from an int64 cumsum; c = 1/2: at most 16 shifted adds.  A piece ends where c_j = 0: at a
    run end, at a masked done, at the last record."""
    g = float(np.float32(gamma))
    c = float(np.float32(np.float32(gamma) * np.float32(lam)))
    H = len(r)
    cut = (1.0 - (np.asarray(done) != 0)) if use_mask else np.ones(H)
    r, v, nv = (np.asarray(x, np.float32).astype(np.float64) for x in (r, v, nv))
    tgt = r + g * nv * cut
    delta = tgt - v
    assert (tgt == np.rint(tgt)).all()
    assert_exact(delta, v, run_end, c)
    stop = (np.asarray(run_end) != 0) | (cut == 0)
    stop[H - 1] = True
    j = np.arange(H)
    last = np.minimum.accumulate(np.where(stop, j, H)[::-1])[::-1]             # the last record of the piece of j
    if c == 1.0:
        P0 = np.concatenate([[0], np.cumsum(delta.astype(np.int64))])
        adv = (P0[last + 1] - P0[:-1]).astype(np.float64)
    else:
        adv = delta.copy()
        for k in range(1, int((last - j).max()) + 1):
            adv[:H - k] += c ** k * delta[k:] * (last[:H - k] >= j[k:])
    ret = adv + v
    for x in (adv, tgt, ret):
        assert (x.astype(np.float32).astype(np.float64) == x).all()
    return adv, tgt, ret
