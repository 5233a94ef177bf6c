"""csrc/minigrid_obs.hip byte for byte against the recording of the reference's observation wrappers
(tests/golden/obs_wrappers.npz) and against tests/obs_ref.py, through every front end: minigrid_obs, TwoarmyVecEnv
(observation=..., goal_direction=...) and the N = 1 facade wrappers of gym_minigrid/wrappers.py.  Every comparison is
byte equality (float64: bit equality, NaN as NaN)."""
import ctypes as C

import numpy as np
import pytest
import torch

import obs_ref as orf
from test_obs_wrappers_cpu import MISSION, NAMES, golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096                                            # guard bytes on either side of an output, a multiple of 16
CONFIGS = [("image", "slope"), ("onehot", "angle"), ("full", None), ("symbolic", "slope"), ("flat", "angle")]


def dev(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return t.to(device=DEV, dtype=dt or t.dtype).contiguous()


def guarded(nbytes):
    g = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert g.data_ptr() % 16 == 0
    return g


def rows_view(g, offset, N, pitch, inner_shape, dtype=torch.uint8):
    """[N, *inner_shape] view of the guarded byte buffer g: rows `pitch` elements apart, the first `offset` bytes behind
    the front guard."""
    item = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(inner_shape))
    flat = g[GUARD + offset:GUARD + offset + ((N - 1) * pitch + n) * item].view(dtype)
    strides, s = [], 1
    for d in reversed(inner_shape):
        strides.insert(0, s)
        s *= d
    return flat.as_strided((N,) + tuple(inner_shape), (pitch,) + tuple(strides))


def expect_rows(nbytes, offset, N, pitch_bytes, rows):
    """The guarded buffer as it must look afterwards: 0xA5 everywhere but the rows' own bytes."""
    want = np.full(GUARD + nbytes + GUARD, 0xA5, np.uint8)
    for e in range(N):
        b = np.ascontiguousarray(rows[e]).view(np.uint8).reshape(-1)
        want[GUARD + offset + e * pitch_bytes:GUARD + offset + e * pitch_bytes + len(b)] = b
    return want


# ------------------------------------------------------------------------------------------------ 1. golden replay
@pytest.mark.parametrize("name", NAMES)
def test_vec_env_replays_the_recording_in_every_kind(name):
    """4 envs take the script's actions; env 0 carries the recorded env id, so its observations are the recorded ones."""
    from twoarmy_amd.vecenv import TwoarmyVecEnv
    z = golden()
    variant, eid = (int(v) for v in z["meta_" + name])
    ops, sel = z["ops_" + name], {int(s): i for i, s in enumerate(z["sel_" + name])}
    for kind, gd in CONFIGS:
        env = TwoarmyVecEnv(variant, num_envs=4, env_id0=eid, policy_actions=False, autoreset=False, observation=kind,
                            goal_direction=gd)
        try:
            step, dirs = 0, []
            for j, op in enumerate(ops):
                if op == -1:
                    obs = env.reset()
                else:
                    obs, _, term, trunc, info = env.step(torch.full((4,), int(op), dtype=torch.int32))
                assert obs.shape[1:] == env.single_observation_shape
                o0 = obs[0].cpu().numpy()
                if kind == "full":
                    assert o0.dtype == np.uint8 and np.array_equal(o0, z["full_" + name][j]), (kind, j)
                elif kind == "symbolic":
                    assert o0.dtype == np.int32 and np.array_equal(o0, z["symbolic_" + name][j]), (kind, j)
                if op == -1:
                    continue
                assert (bool(term[0]), bool(trunc[0])) == (bool(z["term_" + name][step]), bool(z["trunc_" + name][step])), step
                assert "final_observation" not in info
                if gd is not None:
                    assert info["goal_direction"].dtype == torch.float64 and info["goal_direction"].shape == (4,)
                    dirs.append(info["goal_direction"][:1].clone())
                if step in sel:
                    i = sel[step]
                    if kind == "image":
                        assert np.array_equal(o0, z["image_" + name][i]), step
                    elif kind == "onehot":
                        assert o0.dtype == np.uint8 and np.array_equal(o0, z["onehot_" + name][i]), step
                    elif kind == "flat":
                        assert o0.dtype == np.float32 and np.array_equal(o0[:867], z["flatimg_" + name][i].astype(np.float32))
                        assert np.array_equal(o0[867:], z["flat_tail"])
                step += 1
            if gd is not None:
                assert orf.same_f64(torch.cat(dirs).cpu().numpy(), z[gd + "_" + name]), (kind, gd)
        finally:
            env.close()


@pytest.mark.parametrize("name", NAMES)
def test_facade_wrappers_replay_the_recording(name):
    from twoarmy_amd.gym_minigrid import wrappers as W
    from twoarmy_amd.gym_minigrid.envs.twoarmy import Twoarmy_v4, Twoarmy_v6
    z = golden()
    variant, eid = (int(v) for v in z["meta_" + name])
    base = {4: Twoarmy_v4, 6: Twoarmy_v6}[variant](agent_view_size=17, tile_size=17, seed=9981, env_id=eid)
    try:
        onehot, full, symb, flat = W.OneHotPartialObsWrapper(base), W.FullyObsWrapper(base), W.SymbolicObsWrapper(base), \
            W.FlatObsWrapper(base)
        dslope = W.DirectionObsWrapper(base, type="slope")
        dangle = W.DirectionObsWrapper(dslope, type="angle")        # one reset() of the stack resets the env once
        assert onehot.observation_space["image"].shape == (17, 17, 21) and flat.observation_space.shape == (3555,)
        with pytest.raises(TypeError):
            dslope.reset(seed=1)                                    # the reference's reset() takes no kwargs
        with pytest.raises(TypeError):
            dslope.observation({})                                  # goal_position is None before the first reset
        sel = {int(s): i for i, s in enumerate(z["sel_" + name])}
        step, slopes, angles = 0, [], []
        for j, op in enumerate(z["ops_" + name]):
            if op == -1:
                obs = dangle.reset()
                assert "goal_direction" not in obs and dangle.goal_position == dslope.goal_position == (2, 14)
            else:
                obs, _, term, trunc, _ = base.step(int(op))
            assert base.agent_pos + (base.agent_dir,) == tuple(z["agent_" + name][j]), j
            f = full.observation(dict(obs))
            assert f["image"].dtype == np.uint8 and np.array_equal(f["image"], z["full_" + name][j]) and f["mission"] == MISSION
            s = symb.observation(dict(obs))["image"]
            assert s.dtype == np.int64 and np.array_equal(s, z["symbolic_" + name][j]), j
            if op == -1:
                continue
            assert (term, trunc) == (bool(z["term_" + name][step]), bool(z["trunc_" + name][step]))
            slopes.append(dslope.observation(dict(obs))["goal_direction"])
            angles.append(dangle.observation(dict(obs))["goal_direction"])
            assert isinstance(slopes[-1], np.float64)
            if step in sel:
                i = sel[step]
                assert np.array_equal(obs["image"], z["image_" + name][i])
                assert np.array_equal(onehot.observation(dict(obs))["image"], z["onehot_" + name][i])
                fl = flat.observation(dict(obs))
                assert fl.dtype == np.float32 and fl.shape == (3555,)
                assert np.array_equal(fl[:867], z["flatimg_" + name][i].astype(np.float32)) and np.array_equal(fl[867:], z["flat_tail"])
            step += 1
        assert orf.same_f64(np.array(slopes), z["slope_" + name]) and orf.same_f64(np.array(angles), z["angle_" + name])
    finally:
        base.close()


def test_wrapper_plumbing_reset_step_and_reseed():
    from twoarmy_amd.gym_minigrid import wrappers as W
    from twoarmy_amd.gym_minigrid.envs.twoarmy import Twoarmy_v6
    z = golden()
    base = Twoarmy_v6(agent_view_size=17, tile_size=17, seed=9981, env_id=int(z["meta_still"][1]))
    try:
        env = W.ImgObsWrapper(W.FullyObsWrapper(W.ReseedWrapper(base, seeds=[3, 4])))
        assert env.observation_space.shape == (17, 17, 3)
        img = env.reset()
        assert isinstance(img, np.ndarray) and np.array_equal(img, z["full_still"][0])
        img, info = env.reset(return_info=True)
        assert info == {} and np.array_equal(img, z["full_still"][0]) and env.seed_idx == 0
        for j in (1, 2, 3):
            img, r, term, trunc, _ = env.step(int(z["ops_still"][j]))
            assert np.array_equal(img, z["full_still"][j]) and not term and not trunc
        one = W.OneHotPartialObsWrapper(base)
        with pytest.raises(IndexError):
            one.observation({"image": np.full((17, 17, 3), 9, np.uint8)})          # 12 + 9 = 21
    finally:
        base.close()


# ------------------------------------------------------------------------------------------------ 2. synthetic worlds
def test_synthetic_worlds_full_symbolic_onehot():
    from twoarmy_amd import minigrid_obs as mo
    z = golden()
    for i, (W, H) in enumerate([(5, 9), (9, 4)]):
        enc = z["syn%d_grid" % i]
        ag = z["syn%d_agent" % i]
        A = len(ag)
        ty, co, st = (dev(np.repeat(p[None], A, 0)) for p in orf.planes_from_encoded(enc))
        got, err = mo.full_obs(ty, co, st, W, H, dev(ag[:, 0]), dev(ag[:, 1]), dev(ag[:, 2]), want_error=True)
        assert np.array_equal(got.cpu().numpy(), z["syn%d_full" % i]) and not err.any()
        sym = mo.symbolic_obs(ty[:1], W, H)
        assert sym.dtype == torch.int32 and np.array_equal(sym[0].cpu().numpy(), z["syn%d_symbolic" % i])
        oh, err = mo.onehot(dev(enc[None]), want_error=True)
        assert np.array_equal(oh[0].cpu().numpy(), z["syn%d_onehot" % i]) and not err.any()


def test_goal_index_and_direction_on_random_worlds():
    from twoarmy_amd import minigrid_obs as mo
    rs = np.random.RandomState(3)
    for W, H in [(5, 9), (9, 4), (17, 17), (1, 70), (130, 3)]:
        N = 70
        ty = rs.choice([1, 2, 6, 8], (N, W * H), p=[.6, .3, .09, .01]).astype(np.uint8)
        ty[0] = 1                                           # no goal
        ty[1], ty[1, -1] = 1, 8                             # the last cell
        ax, ay = rs.randint(-1, W + 1, N).astype(np.int32), rs.randint(-1, H + 1, N).astype(np.int32)
        k = mo.goal_index(dev(ty), W, H)
        want_k = orf.goal_index(ty, W, H)
        assert np.array_equal(k.cpu().numpy(), want_k) and want_k[0] == -1 and want_k[1] == W * H - 1
        tab = mo.angle_table(W, H, DEV)
        for mode in ("slope", "angle"):
            got, err = mo.goal_direction(k, W, H, dev(ax), dev(ay), mode=mode, table=tab, want_error=True)
            want, werr = orf.goal_direction(want_k, W, H, ax, ay, mode)
            assert np.array_equal(err.cpu().numpy(), werr) and set(werr) == {0, 1, 2}
            assert orf.same_f64(got.cpu().numpy(), want), (W, H, mode)
        assert mo.goal_direction(k, W, H, dev(ax), dev(ay)).shape == (N,)                   # NULL error, no table


# ------------------------------------------------------------------------------------------------ 3. auto-reset
def test_full_observation_under_autoreset_is_the_default_env_plus_the_observation():
    """observation="full" steps without the in-kernel reset, emits, resets the finished envs and emits again: everything
    else must be what the default env returns.  A third env without auto-reset, reset by hand, supplies the pre-reset
    state for the restatement."""
    from twoarmy_amd.vecenv import TwoarmyVecEnv
    from twoarmy_amd._lib import FIELDS
    N, T = 8, 120
    a_env = TwoarmyVecEnv(6, num_envs=N, observation="full")
    b_env = TwoarmyVecEnv(6, num_envs=N)
    c_env = TwoarmyVecEnv(6, num_envs=N, autoreset=False)
    try:
        assert a_env.single_observation_shape == (17, 17, 3) and b_env.single_observation_shape == (17, 17, 3)

        def restate(env):
            ty, co, rec = env.engine.get_state()
            return orf.full(ty, co, None, 17, 17, rec[:, FIELDS["AX"]], rec[:, FIELDS["AY"]], rec[:, FIELDS["DIR"]])[0]
        oa, ob = a_env.reset(), b_env.reset()
        c_env.reset()
        assert np.array_equal(oa.cpu().numpy(), restate(c_env)) and ob.shape == (N, 17, 17, 3)
        acts = torch.from_numpy(np.random.RandomState(5).choice(5, (T, N), p=[.15, .3, .3, .1, .15]))
        ndone = 0
        for t in range(T):
            oa, ra, ta, ua, ia = a_env.step(acts[t])
            ob, rb, tb, ub, ib = b_env.step(acts[t])
            _, _, tc, uc, _ = c_env.step(acts[t])
            assert torch.equal(a_env.engine.gen_obs(), b_env.engine.gen_obs()), t
            assert torch.equal(ra, rb) and torch.equal(ta, tb) and torch.equal(ua, ub), t
            assert torch.equal(a_env.state_matrix, b_env.state_matrix) and torch.equal(a_env.agent_yx, b_env.agent_yx), t
            done = (ta | ua).cpu().numpy()
            assert np.array_equal(done, (tc | uc).cpu().numpy()) and torch.equal(ia["_final_observation"], ib["_final_observation"])
            final = restate(c_env)                                                     # the state the step left
            assert np.array_equal(ia["final_observation"].cpu().numpy()[done], final[done]), t
            c_env.engine.reset(mask=(tc | uc).to(torch.uint8))
            assert np.array_equal(oa.cpu().numpy(), restate(c_env)), t
            assert np.array_equal(restate(a_env), restate(c_env)) and np.array_equal(restate(b_env), restate(c_env)), t
            ndone += int(done.sum())
        assert ndone >= 2 * N                                                          # every env timed out twice at least
    finally:
        a_env.close(); b_env.close(); c_env.close()


# ------------------------------------------------------------------------------------------------ 4. store edges
@pytest.mark.parametrize("n_cells", [1, 9, 49, 289])
@pytest.mark.parametrize("N", [1, 3, 65])
def test_onehot_store_edges(N, n_cells):
    from twoarmy_amd import minigrid_obs as mo
    rs = np.random.RandomState(N * 1000 + n_cells)
    img = np.stack([rs.randint(0, 12, (N, n_cells)), rs.randint(0, 6, (N, n_cells)), rs.randint(0, 3, (N, n_cells))], -1).astype(np.uint8)
    want, _ = orf.onehot(img)
    row = n_cells * 21
    for ipitch in (n_cells * 3, 880 if n_cells == 289 else n_cells * 3 + 13):           # dense; the engine's padded rows
        src = torch.zeros((N, ipitch), dtype=torch.uint8, device=DEV)
        src[:, :n_cells * 3] = dev(img.reshape(N, -1))
        image = src.as_strided((N, n_cells, 3), (ipitch, 3, 1))
        for offset in range(4):
            for pitch in (row, row + 1, row + 37):
                nbytes = offset + N * pitch
                g = guarded(nbytes)
                out = rows_view(g, offset, N, pitch, (n_cells, 21))
                assert mo.onehot(image, out=out) is out
                assert np.array_equal(g.cpu().numpy(), expect_rows(nbytes, offset, N, pitch, want)), (ipitch, offset, pitch)


@pytest.mark.parametrize("n_cells", [1, 9, 49, 289])
@pytest.mark.parametrize("N", [1, 3, 65])
def test_flat_store_edges(N, n_cells):
    """The output is float32, so its base is moved in steps of one float: 0..3 floats (0, 4, 8, 12 bytes) off the
    16-byte alignment of the stores."""
    from twoarmy_amd import minigrid_obs as mo
    rs = np.random.RandomState(N * 1000 + n_cells + 1)
    n_img = n_cells * 3
    img = rs.randint(0, 256, (N, n_img)).astype(np.uint8)
    for n_tail in (2688, 5, 0):
        tail = rs.rand(n_tail).astype(np.float32)
        want = orf.flat(img, tail)
        row = n_img + n_tail
        for ipitch in (n_img, 880 if n_cells == 289 else n_img + 13):
            src = torch.zeros((N, ipitch), dtype=torch.uint8, device=DEV)
            src[:, :n_img] = dev(img)
            image = src.as_strided((N, n_img), (ipitch, 1))
            for off in range(4):
                for pitch in (row, row + 1, row + 7):
                    nbytes = 4 * (off + N * pitch)
                    g = guarded(nbytes)
                    out = rows_view(g, 4 * off, N, pitch, (row,), torch.float32)
                    mo.flat_obs(image, dev(tail) if n_tail else None, out=out)
                    assert np.array_equal(g.cpu().numpy(), expect_rows(nbytes, 4 * off, N, 4 * pitch, want)), (n_tail, ipitch, off, pitch)


@pytest.mark.parametrize("geom", [(5, 9), (9, 4), (17, 17), (40, 37), (1, 1), (3, 700)])
def test_full_and_symbolic_store_edges(geom):
    """(40, 37) and (3, 700): rows of more than 4096 bytes, several workgroups per env in mg_obs_full."""
    from twoarmy_amd import minigrid_obs as mo
    W, H = geom
    N = 3
    rs = np.random.RandomState(W * 100 + H)
    ty, co, st = (rs.randint(0, hi, (N, W * H)).astype(np.uint8) for hi in (10, 6, 3))
    ax = np.array([0, W - 1, W], np.int32)
    ay = np.array([H - 1, 0, 0], np.int32)
    ad = np.array([1, 3, 2], np.int32)
    want, werr = orf.full(ty, co, st, W, H, ax, ay, ad)
    assert list(werr) == [0, 0, 2]
    row = W * H * 3
    for offset in range(4):
        for pitch in (row, row + 5):
            nbytes = offset + N * pitch
            g = guarded(nbytes)
            out = rows_view(g, offset, N, pitch, (W, H, 3))
            _, err = mo.full_obs(dev(ty), dev(co), dev(st), W, H, dev(ax), dev(ay), dev(ad), out=out, want_error=True)
            assert np.array_equal(err.cpu().numpy(), werr)
            assert np.array_equal(g.cpu().numpy(), expect_rows(nbytes, offset, N, pitch, want)), (offset, pitch)
    nost = mo.full_obs(dev(ty), dev(co), None, W, H, dev(ax), dev(ay), dev(ad))                # NULL state, NULL error
    assert np.array_equal(nost.cpu().numpy(), orf.full(ty, co, None, W, H, ax, ay, ad)[0])
    wsym = orf.symbolic(ty, W, H)
    for off in range(4):                                                                        # floats off alignment
        nbytes = 4 * (off + N * row)
        g = guarded(nbytes)
        out = g[GUARD + 4 * off:GUARD + nbytes].view(torch.int32).view(N, W, H, 3)
        mo.symbolic_obs(dev(ty), W, H, out=out)
        assert np.array_equal(g.cpu().numpy(), expect_rows(nbytes, 4 * off, 1, 0, wsym.reshape(1, -1))), off


# ------------------------------------------------------------------------------------------------ 5. index semantics
def test_onehot_index_semantics_and_error():
    from twoarmy_amd import minigrid_obs as mo
    rs = np.random.RandomState(21)
    N, n_cells = 65, 49
    img = np.stack([rs.randint(0, 13, (N, n_cells)), rs.randint(0, 9, (N, n_cells)), rs.randint(0, 4, (N, n_cells))], -1).astype(np.uint8)
    img[:5] = np.minimum(img[:5], (12, 8, 2))                       # envs without an index >= 21
    img[5:9, :, 1] = np.minimum(img[5:9, :, 1], 5)                  # type 12 in the colour field, no error
    img[5:9, :, 2] = np.minimum(img[5:9, :, 2], 2)
    img[5, 0] = (12, 0, 0)
    img[9] = 1
    img[9, -1] = (1, 0, 3)                                          # one bad cell, the last
    img[10] = 1
    img[10, 0] = (255, 255, 255)
    want, werr = orf.onehot(img)
    assert not werr[:9].any() and werr[9] == 1 and werr[10] == 1 and werr.sum() > 20 and want[5, 0].sum() == 2
    got, err = mo.onehot(dev(img), want_error=True)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(err.cpu().numpy(), werr)
    assert not want[10, 0].any()
    assert np.array_equal(mo.onehot(dev(img)).cpu().numpy(), want)                             # NULL error pointer


# ------------------------------------------------------------------------------------------------ 6. arguments
def test_bad_arguments_are_rejected_before_any_launch():
    from twoarmy_amd import _lib
    lib = _lib.lib()
    N, W, H = 3, 5, 9
    u8 = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)                       # noqa: E731
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                             # noqa: E731
    img, oh, pl, fo = u8(N * 27), u8(N * 189), u8(N * W * H), u8(N * W * H * 3)
    i32 = torch.zeros(N * W * H * 3, dtype=torch.int32, device=DEV)
    f32 = torch.zeros(N * 40, dtype=torch.float32, device=DEV)
    f64 = torch.zeros(N, dtype=torch.float64, device=DEV)
    tab = torch.zeros(13 * 9, dtype=torch.float64, device=DEV)
    ag = torch.zeros(N, dtype=torch.int32, device=DEV)
    tl = torch.ones(13, dtype=torch.float32, device=DEV)
    outs, rejected = (oh, fo, i32, f32, f64, ag), []

    def check(fn, good, bad):
        assert fn(*good.values()) == 0
        rejected.extend((fn, {**good, **kw}, kw) for kw in bad)
    check(lib.mg_obs_onehot, dict(image=p(img), ip=0, N=N, n=9, out=p(oh), op=0, err=None, s=None),
          [dict(image=None), dict(out=None), dict(N=0), dict(N=-1), dict(n=0), dict(ip=26), dict(op=188), dict(n=1 << 27)])
    check(lib.mg_obs_full, dict(t=p(pl), c=p(pl), s=None, N=N, W=W, H=H, ax=p(ag), ay=p(ag), ad=p(ag), st=1, out=p(fo), op=0,
                                err=None, stream=None),
          [dict(t=None), dict(c=None), dict(ax=None), dict(ay=None), dict(ad=None), dict(out=None), dict(N=0), dict(W=0),
           dict(H=-1), dict(st=0), dict(op=W * H * 3 - 1), dict(W=1 << 15, H=1 << 15)])
    check(lib.mg_obs_symbolic, dict(t=p(pl), N=N, W=W, H=H, out=p(i32), s=None),
          [dict(t=None), dict(out=None), dict(N=0), dict(W=0), dict(H=0), dict(out=C.c_void_p(i32.data_ptr() + 2)),
           dict(N=1 << 20, W=1 << 10, H=1 << 10)])
    check(lib.mg_obs_flat, dict(image=p(img), ip=0, N=N, n=27, tail=p(tl), nt=13, out=p(f32), op=0, s=None),
          [dict(image=None), dict(out=None), dict(tail=None), dict(N=0), dict(n=0), dict(nt=-1), dict(ip=26), dict(op=39),
           dict(out=C.c_void_p(f32.data_ptr() + 1)), dict(n=1 << 29)])
    check(lib.mg_obs_goal_direction, dict(k=p(i32), N=N, W=W, H=H, ax=p(i32), ay=p(i32), st=1, mode=1, tab=p(tab), out=p(f64),
                                          err=None, s=None),
          [dict(k=None), dict(ax=None), dict(ay=None), dict(out=None), dict(N=0), dict(W=0), dict(H=0), dict(st=0),
           dict(mode=2), dict(mode=-1), dict(tab=None)])
    check(lib.mg_obs_goal_index, dict(t=p(pl), N=N, W=W, H=H, out=p(ag), s=None),
          [dict(t=None), dict(out=None), dict(N=0), dict(W=0), dict(H=0)])
    assert lib.mg_obs_goal_direction(p(i32), N, W, H, p(i32), p(i32), 1, 0, None, p(f64), None, None) == 0   # slope: no table
    assert lib.mg_obs_flat(p(img), 0, N, 27, None, 0, p(f32), 0, None) == 0                               # no tail
    torch.cuda.synchronize()
    before = [t.clone() for t in outs]
    for t in outs:
        t.view(torch.uint8).fill_(0x5A)
    torch.cuda.synchronize()
    for fn, args, kw in rejected:
        assert fn(*args.values()) == -1, (fn.__name__, kw)
    torch.cuda.synchronize()
    assert all((t.view(torch.uint8) == 0x5A).all() for t in outs) and len(before) == len(outs)      # nothing was launched


# ------------------------------------------------------------------------------------------------ 7. view size 7
def test_onehot_and_flat_over_a_7x7_view_with_autoreset():
    from twoarmy_amd.vecenv import TwoarmyVecEnv
    N = 8
    tail = orf.mission_tail(MISSION)
    for kind in ("onehot", "flat"):
        env = TwoarmyVecEnv(6, num_envs=N, agent_view_size=7, observation=kind)
        try:
            restate = (lambda im: orf.onehot(im)[0]) if kind == "onehot" else (lambda im: orf.flat(im, tail))
            assert env.single_observation_shape == ((7, 7, 21) if kind == "onehot" else (7 * 7 * 3 + 2688,))
            init = env._init_obs.cpu().numpy()
            assert np.array_equal(env.reset().cpu().numpy(), restate(init))
            acts = torch.from_numpy(np.random.RandomState(8).randint(0, 5, (60, N)))
            ndone = 0
            for t in range(60):
                obs, _, term, trunc, info = env.step(acts[t])
                image = env._out["obs"].cpu().numpy()
                assert image.shape == (N, 7, 7, 3)
                done = (term | trunc).cpu().numpy()
                assert np.array_equal(info["final_observation"].cpu().numpy(), restate(image)), t
                assert np.array_equal(obs.cpu().numpy(), restate(np.where(done[:, None, None, None], init, image))), t
                ndone += int(done.sum())
            assert ndone >= N
        finally:
            env.close()
