"""numpy restatement of ppo_her_select (include/twoarmy_ppo.h, csrc/ppo_kernels.hip): which first visits of an episode
become hindsight goals, by rule.  Built on oracle/her_oracle.first_visit (np.unique, literally) and
oracle/philox.philox4x32_10; an episode at a time, in plain Python.  tests/test_her_select_cpu.py checks it against things
it does not define itself (her_oracle.relabel on its choices, the meaning of each rule), tests/test_her_select_gpu.py
compares the kernel with it bit for bit.  Also the shared hand-built cases of both files."""
import functools

import numpy as np

from her_oracle import MAX_LEN, first_visit
from philox import philox4x32_10

LATE, KEY16, TABLE = 0, 1, 2
RULES = {"late": LATE, "key16": KEY16, "table": TABLE}
SELECT_TAG = 0x54574F53                     # 'TWOS'
UNREACHABLE = 0xFFFF
F32, U8, I32, I64, U16 = np.float32, np.uint8, np.int32, np.int64, np.uint16


def visit_cell(y, x, width, height):
    """csrc/visit_cell.h: float compares (-0.0 passes as 0), every position outside the grid is the extra bin."""
    y, x = F32(y), F32(x)
    ok = y >= 0 and y < F32(height) and x >= 0 and x < F32(width)
    return int(y) * width + int(x) if ok else width * height


def tie_word(seed, env_id, t1, rank):
    return int(philox4x32_10(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, env_id & 0xFFFFFFFF, t1 & 0xFFFFFFFF,
                             rank & 0xFFFFFFFF, SELECT_TAG)[0])


def select(pos, terminated, truncated, age0, rule, key16=None, table=None, width=17, height=17, seed=0, env_id0=0,
           step0=0, max_goals=4, skip=0, choices=None, stats=None):
    """-> (choices int32[T,N,4], stats int64[6], episodes).  choices / stats: what the arrays hold before the call (a
    copy is updated; None: -1 everywhere / zeros).  episodes: one dict per episode met, handled or not, with what the
    tests ask about: n, s0, t1, L, handled, why, and for handled ones U (first visits among the records skip ..), and
    per candidate idx, rank, key, word, and `picks` = the candidates in pick order as indices into those lists."""
    rule = RULES.get(rule, rule)
    T, N = terminated.shape
    done = (np.asarray(terminated) | np.asarray(truncated)) != 0
    choices = np.full((T, N, 4), -1, I32) if choices is None else np.array(choices, I32)
    stats = np.zeros(6, I64) if stats is None else np.array(stats, I64)
    episodes = []
    for n in range(N):
        start = 0 if int(age0[n]) == 0 else -1
        for t1 in range(T):
            if not done[t1, n]:
                continue
            s0, start = start, t1 + 1
            if s0 < 0:
                episodes.append(dict(n=n, s0=None, t1=t1, L=None, handled=False, why="running at t = 0"))
                continue
            L = t1 - s0 + 1
            if L > MAX_LEN:
                episodes.append(dict(n=n, s0=s0, t1=t1, L=L, handled=False, why="longer than 64"))
                continue
            ep = np.asarray(pos[s0:t1 + 1, n], F32) + F32(0.0)           # -0.0 + 0.0 = +0.0: one position
            fv = first_visit(ep[skip:]) if L > skip else np.zeros(0, np.int64)
            rank = [r for r in range(fv.size) if fv[r] > 0]              # `0 < index`: the first of them is never used
            idx = [int(fv[r]) + skip for r in rank]
            if rule == LATE:
                key = [63 - i for i in idx]
            elif rule == KEY16:
                key = [int(key16[s0 + i, n]) for i in idx]
            else:
                key = [int(table[visit_cell(ep[i, 0], ep[i, 1], width, height)]) for i in idx]
            word = [tie_word(seed, env_id0 + n, step0 + t1, r) for r in rank]
            C = len(rank)
            order = sorted(range(C), key=lambda c: (key[c], word[c], rank[c]))
            k = min(max_goals, C)
            choices[t1, n] = [rank[order[j]] if j < k else -1 for j in range(4)]
            picks = order[:k]
            stats[0] += 1
            stats[1] += C
            stats[2] += k
            stats[3] += sum(idx[c] + 1 for c in picks)
            if rule == KEY16:
                stats[4] += sum(key[c] for c in picks if key[c] != UNREACHABLE)
                stats[5] += sum(1 for c in picks if key[c] == UNREACHABLE)
            elif rule == TABLE:
                stats[4] += sum(key[c] for c in picks)
            episodes.append(dict(n=n, s0=s0, t1=t1, L=L, handled=True, why=None, U=int(fv.size), idx=idx, rank=rank, key=key,
                                 word=word, picks=picks))
        if start < T:
            episodes.append(dict(n=n, s0=None if start < 0 else start, t1=None, L=None, handled=False,
                                 why="not finished at T"))
    return choices, stats, episodes


# ---------------------------------------------------------------------------------------------------- shared cases
CASE_T, CASE_N, SIDE = 70, 5, 17
SENTINEL = -77                               # what `choices` holds before a call wherever the tests look for untouched rows


def _walk(r, L, span):
    """L positions of a random walk over a span x span patch of the grid: short patches make revisits."""
    p = np.zeros((L, 2), F32)
    y, x = r.integers(0, span, 2)
    for i in range(L):
        d = r.integers(0, 5)
        y = min(span - 1, max(0, y + (d == 0) - (d == 1)))
        x = min(span - 1, max(0, x + (d == 2) - (d == 3)))
        p[i] = (y + 3, x + 2)
    return p


@functools.lru_cache(maxsize=None)
def cases():
    """One rollout of 70 steps x 5 envs, built by hand around the edges of the kernel: the 64-row chunk of its walk, the
    64 records of an episode, `skip`, ties, the extra bin.  -> dict of arrays (read-only); check_cases_present() says
    what they hold."""
    r = np.random.default_rng(20260)
    T, N = CASE_T, CASE_N
    pos = np.zeros((T, N, 2), F32)
    term, trunc = np.zeros((T, N), U8), np.zeros((T, N), U8)
    key16 = r.integers(0, 6, (T, N)).astype(U16)                     # few values: ties between pairs everywhere
    ends = {0: [0, 2, 66, 68],                                        # L = 1, 2, 64 (across row 64), 2; then unfinished
            1: [64, 69],                                              # L = 65: skipped; L = 5
            2: [9, 13, 33, 36, 69],                                   # running at t = 0; L = 4, 20, 3, 33
            3: [29, 69],                                              # L = 30, 40
            4: [5, 11, 12, 30, 47, 63, 64]}                           # L = 6, 6, 1, 18, 17, 16 (ends on row 63), 1
    for n, es in ends.items():
        for i, t1 in enumerate(es):
            (term if (n + i) % 2 else trunc)[t1, n] = 1
        term[es[0], n] = trunc[es[0], n] = 1                          # both flags at once
        s0 = 0
        for t1 in es + [T - 1]:
            L = t1 - s0 + 1
            if L > 0:
                pos[s0:t1 + 1, n] = _walk(r, L, 3 if L < 25 else 6)
            s0 = t1 + 1
    pos[3:67, 0] = np.stack([np.arange(64) // 8 + 1, np.arange(64) % 8 + 1], 1)     # 64 distinct cells: lane 63 a candidate
    # env 2, [14, 33]: a +0.0 / -0.0 pair, and every key16 equal: Philox alone orders its candidates
    pos[14:34, 2] = _walk(r, 20, 4) - F32([3, 2])
    pos[16, 2], pos[20, 2] = (0.0, 3.0), (-0.0, 3.0)
    pos[18, 2], pos[23, 2] = (2.0, -0.0), (2.0, 0.0)
    key16[14:34, 2] = 7
    # env 2, [37, 69]: positions outside the world (the extra bin of the table), one of them twice
    pos[40, 2], pos[44, 2], pos[50, 2], pos[51, 2] = (-1.0, 2.0), (17.0, 3.0), (-1.0, 2.0), (4.0, 17.5)
    # env 3, [30, 69]: unreachable keys everywhere but on three records -> some are picked at max_goals = 4, some not
    key16[30:70, 3] = UNREACHABLE
    key16[[35, 41, 52], 3] = (3, 3, 9)
    key16[3:67, 0] = UNREACHABLE                                      # and an episode whose candidates are all unreachable
    key16[5, 4] = UNREACHABLE                                         # and one that sorts behind its episode's other keys
    table = r.integers(-4, 40, SIDE * SIDE + 1).astype(I64)
    table[SIDE * SIDE] = -9                                           # the extra bin sorts first: outside positions are picked
    table[4 * SIDE + 3] = np.int64(-(1 << 40))                        # needs all 64 bits, and the signed compare
    table[5 * SIDE + 4] = np.int64(1 << 41)
    age0 = np.array([0, 0, 7, 0, 0], I32)
    out = dict(pos=pos, terminated=term, truncated=trunc, age0=age0, key16=key16, table=table)
    for a in out.values():
        a.setflags(write=False)
    return out


def run_case(rule, max_goals=4, skip=0, seed=11, env_id0=3, step0=100, stats=None, fill=SENTINEL):
    c = cases()
    return select(c["pos"], c["terminated"], c["truncated"], c["age0"], rule, key16=c["key16"], table=c["table"],
                  width=SIDE, height=SIDE, seed=seed, env_id0=env_id0, step0=step0, max_goals=max_goals, skip=skip,
                  choices=np.full((CASE_T, CASE_N, 4), fill, I32), stats=stats)


@functools.lru_cache(maxsize=None)
def reference(rule, max_goals=4, skip=0, seed=11, env_id0=3, step0=100):
    """run_case, computed once per argument set and shared by the tests (read-only)."""
    ch, st, eps = run_case(rule, max_goals, skip, seed, env_id0, step0)
    ch.setflags(write=False)
    st.setflags(write=False)
    return ch, st, eps


def check_cases_present():
    """Every edge the issue lists really is in the data: asserted on the host before anything is launched."""
    c = cases()
    pos = c["pos"]
    by_rule = {rule: reference(rule)[2] for rule in (LATE, KEY16, TABLE)}
    eps = by_rule[LATE]
    handled = [e for e in eps if e["handled"]]
    assert any(e["L"] == 1 and not e["idx"] for e in handled)                         # length 1: C = 0
    assert any(e["L"] == 2 for e in handled)
    assert any(e["L"] == 64 and e["s0"] < 64 <= e["t1"] and 63 in e["idx"] for e in handled)   # across the chunk, lane 63 live
    assert any(e["L"] == 64 - 48 and e["t1"] == 63 for e in handled)                  # ends on the chunk's last row
    assert any(not e["handled"] and e["why"] == "longer than 64" and e["L"] == 65 for e in eps)
    assert any(not e["handled"] and e["why"] == "running at t = 0" for e in eps)
    assert any(not e["handled"] and e["why"] == "not finished at T" for e in eps)
    for mg in (2, 3, 4):
        assert any(0 < len(e["idx"]) < mg for e in handled), mg                       # C < max_goals
    assert any(len(e["idx"]) > 4 for e in handled)                                    # and more candidates than picks
    assert any(e["U"] < e["L"] for e in handled)                                      # revisits
    for e in reference(LATE, 4, 4)[2]:                                                # skip = 4
        if e["handled"]:
            assert all(i > 4 for i in e["idx"]) and (e["L"] > 5 or not e["idx"])
    sk = [e["L"] for e in reference(LATE, 4, 4)[2] if e["handled"]]
    assert min(sk) < 4 and 4 in sk and 5 in sk and max(sk) == 64
    zero = [e for e in handled if (e["n"], e["s0"], e["t1"]) == (2, 14, 33)][0]         # the +-0.0 pairs: one position each
    for first, again in ((16, 20), (18, 23)):
        assert (pos[first, 2] == pos[again, 2]).all() and np.signbit(pos[first, 2]).any() != np.signbit(pos[again, 2]).any()
        assert again - 14 not in zero["idx"]
    tab = [e for e in by_rule[TABLE] if e["handled"]]
    assert any(e["key"][c] == -9 for e in tab for c in e["picks"])                    # an outside position, picked
    assert any(k < -(1 << 32) for e in tab for k in e["key"]) and any(k > (1 << 32) for e in tab for k in e["key"])
    assert any(e["key"][c] < 0 for e in tab for c in e["picks"])                      # negative table entries
    k16 = [e for e in by_rule[KEY16] if e["handled"]]
    assert any(len(e["key"]) > 4 and len(set(e["key"])) == 1 and e["key"][0] != UNREACHABLE for e in k16)   # all equal
    assert any(1 < len(set(e["key"])) < len(e["key"]) for e in k16)                   # ties between pairs
    picked = [e["key"][c] for e in k16 for c in e["picks"]]
    unpicked = [e["key"][c] for e in k16 for c in range(len(e["key"])) if c not in e["picks"]]
    assert UNREACHABLE in picked and UNREACHABLE in unpicked
    assert any(UNREACHABLE in e["key"] and any(k != UNREACHABLE for k in e["key"]) and
               any(e["key"][c] == UNREACHABLE for c in e["picks"]) for e in k16)      # picked behind reachable ones
