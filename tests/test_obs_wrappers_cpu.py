"""tests/obs_ref.py (the numpy restatement of include/minigrid_obs.h) against every array of tests/golden/obs_wrappers.npz,
the recording of the reference's own observation wrappers (tools/record_obs_golden.py); the host-side mission one-hot;
and the library's exports.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

import obs_ref as orf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSION = "get to the green goal square"


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "obs_wrappers.npz"))
    return {k: z[k] for k in z.files}


NAMES = ["still", "blocked_goal", "walk", "v4_patrol"]


def planes(grids):
    """Grid.encode() [n][W][H][3] -> (type, colour, state) uint8[n][H*W]."""
    p = np.asarray(grids, np.uint8).transpose(0, 2, 1, 3)
    return tuple(np.ascontiguousarray(p[..., k]).reshape(len(grids), -1) for k in range(3))


def step_rows(z, name):
    """Indices into the per-op arrays of the ops that are steps."""
    return np.nonzero(z["ops_" + name] != -1)[0]


def test_the_file_holds_what_the_issue_lists():
    z = golden()
    assert list(z["script_names"]) == NAMES
    assert [int(z["meta_" + n][0]) for n in NAMES] == [6, 6, 6, 4]
    assert tuple(z["goal_position"]) == (2, 14)                       # (k // H, k % W) of the goal at (14, 2)
    sl = np.concatenate([z["slope_" + n] for n in NAMES])
    assert np.isinf(sl).any() and np.isnan(sl).any() and ((sl == 0) & np.signbit(sl)).any()
    assert (z["grid_v4_patrol"][..., 0] == 6).reshape(len(z["grid_v4_patrol"]), -1).sum(1).max() > 3    # patrol balls
    for n in NAMES:
        ends = np.nonzero(z["term_" + n] | z["trunc_" + n])[0]
        assert len(ends) >= 2 and set(ends) <= set(z["sel_" + n]) and set(range(0, len(z["term_" + n]), 8)) <= set(z["sel_" + n])
        assert (z["ops_" + n] == -1).sum() >= 3 and z["ops_" + n][0] == -1
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "obs_wrappers.npz")) <= 434392       # the largest one before


@pytest.mark.parametrize("name", NAMES)
def test_full_and_symbolic_of_every_op(name):
    z = golden()
    ty, co, st = planes(z["grid_" + name])
    assert not st.any()
    ag = z["agent_" + name]
    got, err = orf.full(ty, co, None, 17, 17, ag[:, 0], ag[:, 1], ag[:, 2])
    assert not err.any() and got.dtype == np.uint8 and np.array_equal(got, z["full_" + name])
    sym = orf.symbolic(ty, 17, 17)
    assert np.array_equal(sym, z["symbolic_" + name].astype(np.int32))
    # the quirk: the goal at (14, 2) shows at [2][14], and [14][2] is empty
    assert (sym[:, 2, 14, 2] == 8).all() and (sym[:, 14, 2, 2] == -1).all() and (z["grid_" + name][:, 14, 2, 0] == 8).all()


@pytest.mark.parametrize("name", NAMES)
def test_slope_and_angle_of_every_step_bit_for_bit(name):
    z = golden()
    rows = step_rows(z, name)
    ty = planes(z["grid_" + name])[0]
    k = orf.goal_index(ty[:1], 17, 17)                                # once, at the first reset
    assert k[0] == 2 * 17 + 14
    ag = z["agent_" + name][rows]
    kk = np.repeat(k, len(rows))
    for mode in ("slope", "angle"):
        got, err = orf.goal_direction(kk, 17, 17, ag[:, 0], ag[:, 1], mode)
        assert not err.any() and orf.same_f64(got, z[mode + "_" + name]), mode
    zero_den = ag[:, 0] == 2
    assert np.array_equal(zero_den, ~np.isfinite(z["slope_" + name]))


@pytest.mark.parametrize("name", NAMES)
def test_onehot_and_flat_of_the_sampled_steps(name):
    z = golden()
    img = z["image_" + name]
    oh, err = orf.onehot(img)
    assert not err.any() and np.array_equal(oh, z["onehot_" + name]) and (oh.sum(-1) == 3).all()
    fl = orf.flat(img, z["flat_tail"])
    assert fl.dtype == np.float32 and fl.shape == (len(img), 3555)
    assert np.array_equal(fl[:, :867], z["flatimg_" + name].astype(np.float32)) and np.array_equal(fl[0, 867:], z["flat_tail"])


def test_synthetic_worlds():
    z = golden()
    assert int(z["n_synthetic"]) == 2
    for i, (W, H) in enumerate([(5, 9), (9, 4)]):
        enc = z["syn%d_grid" % i]
        assert enc.shape == (W, H, 3) and set(range(1, 10)) <= set(enc[..., 0].reshape(-1).tolist())
        assert set(enc[enc[..., 0] == 4][:, 2].tolist()) == {0, 1, 2}
        ty, co, st = (p[None] for p in orf.planes_from_encoded(enc))
        ag = z["syn%d_agent" % i]
        A = len(ag)
        got, err = orf.full(np.repeat(ty, A, 0), np.repeat(co, A, 0), np.repeat(st, A, 0), W, H, ag[:, 0], ag[:, 1], ag[:, 2])
        assert not err.any() and np.array_equal(got, z["syn%d_full" % i])
        assert np.array_equal(orf.symbolic(ty, W, H)[0], z["syn%d_symbolic" % i].astype(np.int32))
        oh, err = orf.onehot(enc[None])
        assert not err.any() and np.array_equal(oh[0], z["syn%d_onehot" % i])


def test_index_semantics_and_errors_of_the_restatement():
    img = np.array([[[12, 0, 0], [20, 5, 2], [21, 0, 0], [1, 9, 0], [1, 8, 0], [1, 0, 3], [2, 6, 1]]], np.uint8)
    oh, err = orf.onehot(img)
    assert err[0] == 1
    assert sorted(np.nonzero(oh[0, 0])[0]) == [12, 18] and sorted(np.nonzero(oh[0, 1])[0]) == [17, 20]
    assert sorted(np.nonzero(oh[0, 2])[0]) == [12, 18] and sorted(np.nonzero(oh[0, 3])[0]) == [1, 18]
    assert sorted(np.nonzero(oh[0, 4])[0]) == [1, 18, 20] and sorted(np.nonzero(oh[0, 5])[0]) == [1, 12]
    assert sorted(np.nonzero(oh[0, 6])[0]) == [2, 18, 19]
    assert orf.onehot(img[:, 4:5])[1][0] == 0
    t = np.ones((2, 12), np.uint8)
    got, err = orf.full(t, t * 0, None, 4, 3, [4, 0], [0, -1], [0, 0])
    assert list(err) == [2, 2] and (got == (1, 0, 0)).all()
    out, err = orf.goal_direction(np.array([-1, 5, 5]), 4, 3, [0, 0, 4], [0, 0, 0])
    assert list(err) == [1, 0, 2] and np.isnan(out[[0, 2]]).all() and out[1] == np.divide(5 % 4 - 0, 5 // 3 - 0)


def test_mission_tail():
    from twoarmy_amd import minigrid_obs
    z = golden()
    tail = minigrid_obs.mission_tail(MISSION)
    assert tail.dtype == np.float32 and np.array_equal(tail, z["flat_tail"]) and np.array_equal(tail, orf.mission_tail(MISSION))
    assert tail.sum() == len(MISSION) and tail.reshape(96, 28)[3, 26] == 1
    assert minigrid_obs.mission_tail("A, b").reshape(96, 28)[:4].argmax(1).tolist() == [0, 27, 26, 1]
    with pytest.raises(ValueError):
        minigrid_obs.mission_tail("!")
    with pytest.raises(AssertionError):
        minigrid_obs.mission_tail("a" * 97)
    assert minigrid_obs.mission_tail("a" * 96).sum() == 96


def test_library_exports_the_observation_abi_and_the_front_end_imports():
    import __graft_entry__ as ge
    ge.build()
    import twoarmy_amd
    from twoarmy_amd import minigrid_obs
    txt = open(os.path.join(ROOT, "include", "minigrid_obs.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mg_obs_[a-z0-9_]+)\s*\(", txt))
    assert declared == {"mg_obs_onehot", "mg_obs_full", "mg_obs_symbolic", "mg_obs_flat", "mg_obs_goal_index",
                        "mg_obs_angle_table_size", "mg_obs_goal_direction"}
    lib = twoarmy_amd._lib.lib()
    for s in declared:
        assert hasattr(lib, s) and s in twoarmy_amd._lib.exported_symbols(), s
    assert lib.mg_obs_angle_table_size(17, 17) == 33 * 33 and lib.mg_obs_angle_table_size(5, 9) == 13 * 9
    assert lib.mg_obs_angle_table_size(0, 3) == -1
    tab = minigrid_obs.angle_table(5, 9).numpy().reshape(13, 9)      # host table: [p + H - 1][q + W - 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        assert orf.same_f64(tab[-8 + 8, 0 + 4], np.arctan(np.divide(-8, 0))) and np.isnan(tab[8, 4])
        assert tab[4 + 8, -4 + 4] == np.arctan(np.divide(4, -4)) and tab[8, 0] == 0 and np.signbit(tab[8, 0])
    for f in ("onehot", "full_obs", "symbolic_obs", "flat_obs", "mission_tail", "goal_index", "goal_direction"):
        assert callable(getattr(minigrid_obs, f))
