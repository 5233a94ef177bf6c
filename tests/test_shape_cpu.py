"""Host-side checks of the reward shaping of include/minigrid_nav.h: the numpy reference (shape_ref.py) against answers
written out by hand, the telescoping sum, the terminal rule, the pass-through of unshaped rewards, the header's flag values
against the front end's constants, and the argument errors of the trainer and the command line that need no device."""
import os
import re
import types

import numpy as np
import pytest

import nav_ref
import shape_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = nav_ref.UNREACHABLE
W, H = 5, 4
GOAL = (4, 1)                                                     # (x, y)


def world():
    """5 x 4, empty but for one wall at (2, 1), right between the start column and the goal."""
    ty = np.ones((H, W), np.uint8)
    ty[1, 2] = 2
    return ty.reshape(1, -1)


def centre(x, y):
    return (y + 0.5, x + 0.5)                                     # positions are (y, x)


def test_the_field_of_the_small_world():
    d = nav_ref.field(world()[0], None, W, H, goal=GOAL)["dist"].reshape(H, W)
    assert d.tolist() == [[5, 4, 3, 2, 1], [6, 5, U, 1, 0], [5, 4, 3, 2, 1], [6, 5, 4, 3, 2]]


# (before (x, y), after (x, y) or a position, done) -> (F, mask) without the flag, (F, mask) with it;  scale = gamma = 0.5
KNOWN = [
    (((1, 1), (1, 0), 0), (1.5, 1), (1.5, 1)),                    # 5 -> 4: 0.5 * -2 - -2.5
    (((1, 0), (1, 1), 0), (0.75, 1), (0.75, 1)),                  # 4 -> 5: 0.5 * -2.5 - -2
    (((3, 1), (4, 1), 0), (0.5, 1), (0.5, 1)),                    # onto the goal: phi_after = 0
    (((3, 1), (4, 1), 1), (0.5, 1), (0.5, 1)),                    # ... and done: the same
    (((4, 1), (4, 1), 0), (0.0, 1), (0.0, 1)),                    # standing on the goal: shaped, F = 0
    (((0, 3), (0, 3), 1), (1.5, 1), (3.0, 1)),                    # cut off at distance 6: 0.5 * -3 - -3 / 0 - -3
    (((1, 1), (2, 1), 0), (0.0, 0), (0.0, 0)),                    # after state on the wall: unshaped
    (((1, 1), (2, 1), 1), (0.0, 0), (2.5, 1)),                    # ... unless the step was terminal: 0 - -2.5
    (((2, 1), (1, 1), 0), (0.0, 0), (0.0, 0)),                    # acting state on the wall
    (((2, 1), (1, 1), 1), (0.0, 0), (0.0, 0)),                    # ... terminal or not
    (((1, 1), None, 0), (0.0, 0), (0.0, 0)),                      # after position outside the world
    (((1, 1), None, 1), (0.0, 0), (2.5, 1)),
]


@pytest.mark.parametrize("flags", [0, shape_ref.ZERO_TERMINAL])
def test_known_answers(flags):
    dist = nav_ref.fields(world(), None, W, H, goal=([GOAL[0]], [GOAL[1]]))[0]
    T = len(KNOWN)
    before = np.array([[centre(*k[0][0])] for k in KNOWN], np.float32)
    after = np.array([[centre(*k[0][1]) if k[0][1] is not None else (np.nan, 1.0)] for k in KNOWN], np.float32)
    done = np.array([[k[0][2]] for k in KNOWN], np.uint8)
    reward = np.full((T, 1), 0.25, np.float32)
    out, f, mask = shape_ref.shape(dist, before, after, W, H, reward, done=done, scale=0.5, gamma=0.5, flags=flags)
    want = [k[2 if flags else 1] for k in KNOWN]
    assert f.dtype == np.float32 and out.dtype == np.float32 and mask.dtype == np.uint8
    assert f[:, 0].tolist() == [w[0] for w in want] and mask[:, 0].tolist() == [w[1] for w in want]
    assert out[:, 0].tolist() == [0.25 + w[0] for w in want]
    assert shape_ref.shape(dist, before, after, W, H, None, done=done, scale=0.5, gamma=0.5, flags=flags)[0] is None


def test_the_age_rule_moves_the_acting_position_only():
    dist = nav_ref.fields(world(), None, W, H, goal=([GOAL[0]], [GOAL[1]]))[0]
    before = np.array([[centre(0, 3)], [centre(0, 3)], [centre(0, 3)]], np.float32)
    after = np.array([[centre(0, 2)]] * 3, np.float32)
    age = np.array([[1], [0], [-3]], np.int32)
    init = np.array(centre(3, 1), np.float32)                     # distance 1
    _, f, mask = shape_ref.shape(dist, before, after, W, H, None, age, init, scale=1.0, gamma=1.0)
    assert f[:, 0].tolist() == [1.0, -4.0, -4.0] and mask[:, 0].tolist() == [1, 1, 1]     # 6 -> 5;  1 -> 5


def test_rounding_is_per_operation():
    """scale * d, gamma * phi and the difference are each rounded to float32: the answers differ from the exact ones."""
    d_b, d_a = np.array([7]), np.array([3])
    f, _ = shape_ref.terms(d_b, d_a, None, 0.01, 0.99, False)
    m_b, m_a = np.float32(0.01) * np.float32(7), np.float32(0.01) * np.float32(3)
    want = np.float32(np.float32(0.99) * -m_a) - -m_b
    assert f[0] == want and f.dtype == np.float32
    exact = np.float64(np.float32(0.99)) * -(np.float64(np.float32(0.01)) * 3) + np.float64(np.float32(0.01)) * 7
    assert np.float64(f[0]) != exact                              # a fused or a double evaluation would show


def test_telescoping():
    """gamma = 1, scale = 2^-3: every F is scale * (d_before - d_after) exactly, so the sum over a run of shaped steps in
    which each step starts where the last one ended is scale * (d_first - d_last), in float32 arithmetic and exactly."""
    rng = np.random.default_rng(5)
    Ww = Hh = 17
    ty = np.where(rng.random(Ww * Hh) < 0.15, 2, 1).astype(np.uint8)
    ty[0] = 1
    dist = nav_ref.fields(ty[None], None, Ww, Hh, goal=([0], [0]))[0]
    cells = np.flatnonzero(dist[0] != U)
    runs = 0
    for start in cells[:: max(1, len(cells) // 12)]:
        path, c = [int(start)], int(start)
        for _ in range(40):                                       # a random walk over reachable cells
            x, y = c % Ww, c // Ww
            nb = [(x + dx) + (y + dy) * Ww for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1), (0, 0))
                  if 0 <= x + dx < Ww and 0 <= y + dy < Hh and dist[0, (x + dx) + (y + dy) * Ww] != U]
            c = int(nb[rng.integers(0, len(nb))])
            path.append(c)
        pos = np.array([[(c // Ww + 0.5, c % Ww + 0.5)] for c in path], np.float32)
        _, f, mask = shape_ref.shape(dist, pos[:-1], pos[1:], Ww, Hh, None, scale=0.125, gamma=1.0)
        assert mask.all()
        for a, b in ((0, 40), (3, 17), (39, 40)):
            total = np.float32(0.0)
            for v in f[a:b, 0]:
                total = np.float32(total + v)
            assert total == np.float32(0.125) * (np.float32(dist[0, path[a]]) - np.float32(dist[0, path[b]]))
        runs += 1
    assert runs >= 10


def test_zero_terminal_rule():
    d_b = np.array([4, 4, U, U, 0, 2])
    d_a = np.array([3, U, 3, U, 0, U])
    done = np.array([1, 1, 1, 1, 1, 0], np.uint8)
    f0, m0 = shape_ref.terms(d_b, d_a, done, 1.0, 0.5, False)
    assert m0.tolist() == [1, 0, 0, 0, 1, 0] and f0.tolist() == [2.5, 0.0, 0.0, 0.0, 0.0, 0.0]
    f1, m1 = shape_ref.terms(d_b, d_a, done, 1.0, 0.5, True)      # done: phi_after = 0, shaped iff the acting state is reachable
    assert m1.tolist() == [1, 1, 0, 0, 1, 0] and f1.tolist() == [4.0, 4.0, 0.0, 0.0, 0.0, 0.0]
    assert not np.signbit(f0).any() and not np.signbit(f1).any()  # an unshaped F is +0.0


def test_unshaped_rewards_pass_through_bit_for_bit():
    bits = np.array([0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000001, 0x3F800000], np.uint32)
    reward = bits.view(np.float32)
    f = np.full(6, 0.5, np.float32)
    out = shape_ref.apply(reward, f, np.zeros(6, np.uint8))
    assert out.view(np.uint32).tolist() == bits.tolist()
    shaped = shape_ref.apply(reward, f, np.ones(6, np.uint8))
    assert shaped[0] == 0.5 and shaped[5] == 1.5 and np.isnan(shaped[1:4]).all()
    assert shape_ref.apply(np.array([-0.0], np.float32), np.array([0.0], np.float32), np.ones(1, np.uint8)).view(np.uint32)[0] == 0


def test_goal_reference_is_the_field_reference_for_a_shared_goal():
    """The invariant of mg_nav_goal_shape on the host."""
    rng = np.random.default_rng(9)
    N, T, Ww, Hh = 3, 6, 9, 4
    ty = np.stack([nav_ref.random_world(rng, Ww, Hh, 0.2)[0] for _ in range(N)])
    st = np.zeros_like(ty)
    gc = rng.integers(0, Ww * Hh, N)
    c = rng.integers(0, Ww * Hh, (2, T, N))
    before = np.stack([c[0] // Ww + 0.5, c[0] % Ww + 0.5], -1).astype(np.float32)
    after = np.stack([c[1] // Ww + 0.5, c[1] % Ww + 0.5], -1).astype(np.float32)
    after[2, 1] = (np.nan, 0.0)
    age = rng.integers(-1, 3, (T, N)).astype(np.int32)
    init = np.array([0.5, 0.5], np.float32)
    done = (rng.random((T, N)) < 0.3).astype(np.uint8)
    reward = rng.standard_normal((T, N)).astype(np.float32)
    dist = nav_ref.fields(ty, st, Ww, Hh, goal=(gc % Ww, gc // Ww))[0]
    order = rng.permutation(T * N)
    t, n = order // N, order % N
    goal = np.stack([gc[n] // Ww + 0.25, gc[n] % Ww + 0.75], 1).astype(np.float32)
    for flags in (0, shape_ref.ZERO_TERMINAL):
        want = shape_ref.shape(dist, before, after, Ww, Hh, reward, age, init, done, 0.01, 0.99, flags)
        got = shape_ref.goal_shape(ty, st, Ww, Hh, t, n, goal, before, after, reward[t, n], done[t, n], age, init,
                                   flags=flags, scale=0.01, gamma=0.99)
        for g, w in zip(got, want):
            assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                                  w[t, n].view(np.uint32) if w.dtype == np.float32 else w[t, n])
        assert got[2].any() and not got[2].all()


def test_header_flags_and_arguments():
    import twoarmy_amd
    from twoarmy_amd import minigrid_nav as nav
    header = open(os.path.join(ROOT, "include", "minigrid_nav.h")).read()
    defs = {k: int(v, 0) for k, v in re.findall(r"#define (MG_NAV_\w+) +(-?\w+)", header) if re.match(r"-?(0x)?[0-9A-Fa-f]+$", v)}
    assert defs["MG_NAV_SHAPE_ZERO_TERMINAL"] == nav.SHAPE_ZERO_TERMINAL == shape_ref.ZERO_TERMINAL == 2
    assert defs["MG_NAV_DOORS_OPEN"] == nav.DOORS_OPEN == nav_ref.DOORS_OPEN == 1
    assert nav.SHAPE_ZERO_TERMINAL & nav.DOORS_OPEN == 0          # one flag space
    assert defs["MG_NAV_UNREACHABLE"] == nav.UNREACHABLE == U
    txt = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {"mg_nav_shape": "dist dist_pitch period n_envs width height pos_before pos_after age init_pos done reward T "
                            "scale gamma flags reward_out shaping mask stream",
            "mg_nav_goal_shape": "type state n_envs width height pass_types flags rec_t rec_n rec_goal rec_done rec_reward "
                                 "n_records pos_before pos_after age init_pos T scale gamma reward_out shaping mask stream"}
    for name, names in want.items():
        args = [a.strip() for a in re.search(r"\b%s\s*\((.*?)\);" % name, txt, re.S).group(1).split(",")]
        assert [re.search(r"(\w+)$", a).group(1) for a in args] == names.split(), name
        assert len(twoarmy_amd._lib._SIGS[name][1]) == len(args) and name in twoarmy_amd._lib.exported_symbols()
    for word in ("one rounding", "NaN payload stays", "phi_after = 0", "depends on record b alone", "reward_out == reward"):
        assert word in header[header.index("Reward shaping"):], word


def test_enable_shaping_argument_errors_need_no_device():
    from twoarmy_amd.soa import train_ppo
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    for bad in (0, 0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="positive finite"):
            VecPPOTrainer.enable_shaping(types.SimpleNamespace(), bad)                       # before anything is touched
    with pytest.raises(ValueError, match="booleans"):
        VecPPOTrainer.enable_shaping(types.SimpleNamespace(), 0.1, hindsight="yes")
    with pytest.raises(ValueError, match="booleans"):
        VecPPOTrainer.enable_shaping(types.SimpleNamespace(), 0.1, timed=1)
    with pytest.raises(RuntimeError, match="before enable_shaping"):
        VecPPOTrainer.shape_potential(types.SimpleNamespace(shaping=None))
    with pytest.raises(RuntimeError, match="before enable_shaping"):
        VecPPOTrainer.shaping_stats(types.SimpleNamespace(shaping=None))
    with pytest.raises(SystemExit, match="need --shaping_scale"):
        train_ppo.main(["--shaping_timed"])
    with pytest.raises(SystemExit, match="need --shaping_scale"):
        train_ppo.main(["--shaping_no_hindsight"])
    with pytest.raises(SystemExit, match="finite number >= 0"):
        train_ppo.main(["--shaping_scale", "-1"])
    args = train_ppo.build_parser().parse_args(["--shaping_scale", "0.05", "--shaping_timed"])
    assert args.shaping_scale == 0.05 and args.shaping_timed and not args.shaping_no_hindsight
    assert train_ppo.build_parser().parse_args([]).shaping_scale == 0.0
    ss = {"mean": 0.01234, "unshaped": 0.25, "her_mean": None, "her_unshaped": None}
    assert train_ppo.shaping_fields(ss, False) == " shaping mean 0.0123 unshaped 0.2500"
    assert train_ppo.shaping_fields(ss, True).endswith(" her shaping mean - her unshaped -")
