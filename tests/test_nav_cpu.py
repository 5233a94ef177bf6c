"""Host-side checks of the distance fields (include/minigrid_nav.h): the test reference against an independent
formulation, the Twoarmy reset world, and the header's constants against the code they restate."""
import glob
import os
import re

import numpy as np
import pytest

import nav_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 7), (7, 1), (5, 9), (9, 4), (17, 17), (31, 32), (32, 32)]          # (W, H)
DENSITIES = [0.0, 0.2, 0.45]


def _header():
    return open(os.path.join(ROOT, "include", "minigrid_nav.h")).read()


def _define(name):
    return int(re.search(r"#define %s\s+(\(?-?\w+\)?)" % name, _header()).group(1).strip("()"), 0)


@pytest.mark.parametrize("W,H", SIZES)
def test_bfs_equals_relaxation_on_random_worlds(W, H):
    """About 200 worlds in all: 8 sizes x 3 wall densities x 9 worlds, every type code 0..17 and doors in all three
    states present, both source modes, three pass masks and the doors-open flag."""
    rng = np.random.default_rng(1000 * W + H)
    seen_types, seen_door_states = set(), set()
    for dens in DENSITIES:
        for k in range(9):
            ty, st = nav_ref.random_world(rng, W, H, dens)
            if W * H >= 18 and k == 0:                       # every type code at least once per size
                ty[rng.permutation(W * H)[:18]] = np.arange(18)
                st[ty == 4] = rng.integers(0, 3, int((ty == 4).sum()))
            for g in rng.integers(0, W * H, k % 4):          # 0..3 goal cells
                ty[g] = 8
            seen_types |= set(ty.tolist())
            seen_door_states |= set(st[ty == 4].tolist())
            pass_types = [nav_ref.PASS_DEFAULT, nav_ref.PASS_DEFAULT & ~(1 << 9), nav_ref.PASS_DEFAULT | (1 << 6)][k % 3]
            flags = nav_ref.DOORS_OPEN if k % 4 == 3 else 0
            state = None if k % 5 == 4 else st
            goal = None if k % 2 == 0 else (int(rng.integers(0, W)), int(rng.integers(0, H)))
            a = nav_ref.field(ty, state, W, H, pass_types, flags, goal)
            b = nav_ref.relax(ty, state, W, H, pass_types, flags, goal)
            assert np.array_equal(a["dist"].astype(np.int64), b), (W, H, dens, k)
            finite = b[b != nav_ref.UNREACHABLE]
            assert a["error"] == (0 if finite.size else 1)
            assert a["depth"] == (finite.max() if finite.size else 0)
    if W * H >= 18:
        assert seen_types >= set(range(18))
    if W * H >= 100:
        assert seen_door_states == {0, 1, 2}


def test_expert_action_and_error_codes_of_the_reference():
    W = H = 5
    ty = np.ones(W * H, np.uint8)
    r = nav_ref.field(ty, None, W, H, goal=(2, 2), agent=(4, 4))
    assert (r["agent_dist"], r["agent_action"], r["error"]) == (4, 0, 0)          # left before up
    r = nav_ref.field(ty, None, W, H, goal=(2, 2), agent=(0, 0))
    assert (r["agent_dist"], r["agent_action"]) == (4, 1)                         # right before down
    r = nav_ref.field(ty, None, W, H, goal=(2, 2), agent=(2, 2))
    assert (r["agent_dist"], r["agent_action"]) == (0, 6)
    r = nav_ref.field(ty, None, W, H, goal=(5, 2), agent=(2, 2))
    assert r["error"] == 2 and (r["dist"] == nav_ref.UNREACHABLE).all() and r["agent_action"] == -1
    r = nav_ref.field(ty, None, W, H, agent=(2, 2))
    assert r["error"] == 1 and (r["dist"] == nav_ref.UNREACHABLE).all()
    r = nav_ref.field(ty, None, W, H, goal=(2, 2), agent=(-1, 2))
    assert r["error"] == 3 and r["agent_dist"] == nav_ref.UNREACHABLE and r["agent_action"] == -1
    assert r["dist"].reshape(H, W)[0, 0] == 4


def test_serpentine_is_longer_than_a_byte():
    for W, H in ((32, 32), (31, 32)):
        ty, src = nav_ref.serpentine(W, H)
        r = nav_ref.field(ty, None, W, H, goal=src)
        assert r["depth"] > 255 and r["depth"] >= W * H // 2 - W, (W, H, r["depth"])


def test_twoarmy_reset_world_has_a_finite_start_to_goal_distance():
    from golden_util import load_traces
    traces, _ = load_traces()
    seen, resets = set(), 0
    for tr in traces:
        rows = np.nonzero(tr["op"] == -1)[0].tolist()        # the reset rows; row 0 is the world after the first step
        resets += len(rows)
        for i in sorted(set(rows + [0])):
            grid = tr["grid"][i]                             # Grid.encode(): [x][y][3]
            ty = np.ascontiguousarray(grid[:, :, 0].T).reshape(-1)
            st = np.ascontiguousarray(grid[:, :, 2].T).reshape(-1)
            assert (ty == 8).sum() == 1
            ax, ay = (int(v) for v in tr["agent"][i])
            r = nav_ref.field(ty, st, 17, 17, agent=(ax, ay))
            assert r["error"] == 0 and 0 < r["agent_dist"] < nav_ref.UNREACHABLE and r["agent_action"] in (0, 1, 2, 3)
            static = nav_ref.field(ty, st, 17, 17, nav_ref.PASS_DEFAULT | (1 << 6), agent=(ax, ay))
            assert static["agent_dist"] <= r["agent_dist"]
            if i in rows:
                assert (ax, ay) == (3, 15) and static["agent_dist"] == 24, (ax, ay, static["agent_dist"])
            seen.add(int(tr["variant"]))
    assert resets >= 1
    assert seen == {4, 6}


def test_pass_default_is_the_rule_of_mg_step():
    """The types mg_step_kernel lets the agent onto, read out of its source, are the bits of MG_NAV_PASS_DEFAULT."""
    src = open(glob.glob(os.path.join(ROOT, "goal-*_amd", "csrc", "minigrid_view.hip"))[0]).read()
    consts = dict(re.findall(r"\b(T_[A-Z]+) = (\d+)", src))
    body = src[src.index("void mg_step_kernel"):]
    stmt = re.search(r"const bool overlap = (.*?);", body, re.S).group(1)
    main, door = stmt.split("(t == T_DOOR")
    assert re.fullmatch(r"\s*&& \(state \? state\[o\] : 0\) == 0\)\s*", door), door     # doors: open ones only
    types = set()
    for term in main.split("||"):
        term = term.strip()
        if not term:
            continue
        m = re.fullmatch(r"t (<=|==) (\w+?)u?", term)
        assert m, term
        v = int(consts.get(m.group(2), m.group(2)))
        types |= set(range(v + 1)) if m.group(1) == "<=" else {v}
    types.add(int(consts["T_DOOR"]))
    assert types == {0, 1, 3, 4, 8, 9, 11}
    assert _define("MG_NAV_PASS_DEFAULT") == sum(1 << t for t in types) == nav_ref.PASS_DEFAULT
    assert _define("MG_NAV_UNREACHABLE") == nav_ref.UNREACHABLE == 0xFFFF
    assert _define("MG_NAV_DOORS_OPEN") == nav_ref.DOORS_OPEN
    assert _define("MG_NAV_MAX_SIDE") == 32


def test_front_end_constants_and_exported_symbols():
    import twoarmy_amd
    from twoarmy_amd import minigrid_nav as nav
    syms = twoarmy_amd._lib.exported_symbols()
    assert "mg_nav_field" in syms and "mg_nav_lookup" in syms
    assert nav.PASS_DEFAULT == _define("MG_NAV_PASS_DEFAULT") and nav.UNREACHABLE == _define("MG_NAV_UNREACHABLE")
    assert nav.DOORS_OPEN == _define("MG_NAV_DOORS_OPEN") and nav.MAX_SIDE == _define("MG_NAV_MAX_SIDE")
    assert nav.ACTION_STAY == _define("MG_NAV_ACTION_STAY") and nav.ACTION_NONE == _define("MG_NAV_ACTION_NONE")
    # the ctypes signatures have the header's argument counts
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("mg_nav_field", "mg_nav_lookup"):
        args = re.search(r"\b%s\s*\((.*?)\);" % name, txt, re.S).group(1)
        assert len(twoarmy_amd._lib._SIGS[name][1]) == len(args.split(",")), name
