"""The agent-view frame without a GPU: the numpy restatement (tests/pov_ref.py) against every frame recorded from the
reference's get_pov_render (tests/golden/pov.npz, tools/record_pov_golden.py) byte for byte, the host side of
mg_render_pov (exported symbol, argument rejection), and the pixel wrappers' declared spaces and side effects against
the recording.

The occlusion worlds hold lava, which the device renderer does not draw (include/minigrid_render.h: error 1, an empty
tile in its place).  102 of the 480 recorded world frames show a lava cell; in those every byte outside the lava tiles
is compared, the error flag must be 1 and the lava tiles are the empty tile.  The other 378 frames and all 59 script
frames are compared whole, with error 0."""
import ctypes as C
import types

import numpy as np

import pov_ref as pr
import render_ref as rr

VIEWS = ((3, 8), (7, 8), (3, 1), (3, 3))


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import twoarmy_amd
    return twoarmy_amd._lib.lib()


def test_restatement_equals_every_recorded_world_frame():
    z = pr.load_golden()
    n = int(z["n_worlds"])
    assert n == 30
    hidden = carried = whole = 0
    two_sides = set()
    for c in range(n):
        ty, co, st, W, H, ax, ay, carry = pr.world_planes(c)
        carried += int(carry[0] != 0)
        for V, ts in VIEWS:
            vis, ref = z["w_vis_%02d_%d" % (c, V)], z["w_pov_%02d_%d_%d" % (c, V, ts)]
            assert ref.shape == (4, V * ts, V * ts, 3)
            a = ([ty] * 4, [co] * 4, [st] * 4, W, H, [ax] * 4, [ay] * 4, range(4), V, ts, [carry] * 4, vis)
            got, err = pr.pov_frames(*a)
            skip = pr.undrawn_pixels(*a)
            for d in range(4):
                assert err[d] == int(skip[d].any())
                whole += int(not err[d])
                diff = (got[d] != ref[d]).any(axis=2)
                assert not (diff & ~skip[d]).any(), "world %d V=%d ts=%d dir %d: %d pixels differ" % (
                    c, V, ts, d, int((diff & ~skip[d]).sum()))
            hidden += int((vis == 0).sum())
        for d in range(4):                                 # the 7 x 7 window of get_view_exts against the world's edges
            tx = ax if d == 0 else (ax - 6 if d == 2 else ax - 3)
            ty_ = ay if d == 1 else (ay - 6 if d == 3 else ay - 3)
            if (tx < 0 or tx + 7 > W) and (ty_ < 0 or ty_ + 7 > H):
                two_sides.add(d)
    assert hidden > 0 and carried == 6 and two_sides == {0, 1, 2, 3} and whole == 378


def test_restatement_equals_every_recorded_script_frame():
    z = pr.load_golden()
    names = [str(n) for n in z["script_names"]]
    assert names == ["K4_goal", "K5_ball_onto_agent"]
    g = rr.load_golden()
    term = trunc = 0
    for name in names:
        variant, eid, V, ts = (int(v) for v in z["s_meta_" + name])
        assert (V, ts) == (7, 8)
        frames, agents, grids = pr.load_script(name), z["s_agents_" + name], g["grids_" + name]
        assert np.array_equal(z["s_ops_" + name], g["ops_" + name]) and np.array_equal(agents, g["agents_" + name])
        assert len(frames) == len(grids) == len(z["s_ops_" + name]) + 1
        p = np.ascontiguousarray(np.transpose(grids, (0, 2, 1, 3))).reshape(len(grids), 289, 3)
        got, err = pr.pov_frames(p[..., 0], p[..., 1], p[..., 2], 17, 17, agents[:, 0], agents[:, 1], agents[:, 2], V, ts)
        assert not err.any()
        for t in range(len(frames)):
            assert np.array_equal(got[t], frames[t]), "%s frame %d: %d bytes differ" % (name, t, int((got[t] != frames[t]).sum()))
        term += int(z["s_done_" + name][:, 0].any())
        trunc += int(z["s_done_" + name][:, 1].any())
    assert term and trunc                                  # the two scripts end one episode each way


def test_exported_symbol():
    lib = _lib()
    import twoarmy_amd
    assert hasattr(lib, "mg_render_pov") and "mg_render_pov" in twoarmy_amd._lib.exported_symbols()


def test_argument_rejection_needs_no_device():
    lib = _lib()
    p = C.c_void_p(4096)                                # never dereferenced: every call below fails before a launch
    ok = dict(type=p, colour=p, state=None, n_envs=4, width=17, height=17, ax=p, ay=p, ad=p, stride=1, carrying=None,
              env_index=None, n_out=4, vis=None, V=7, atlas=p, ts=8, frame=p, pitch=0, error=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mg_render_pov(*[a[k] for k in ok])
    for kw in (dict(type=None), dict(colour=None), dict(ax=None), dict(ay=None), dict(ad=None), dict(atlas=None),
               dict(frame=None), dict(n_envs=0), dict(width=0), dict(height=-1), dict(n_out=0), dict(stride=0),
               dict(ts=0), dict(ts=257), dict(n_out=5), dict(V=0), dict(V=32), dict(V=-7),
               dict(pitch=7 * 7 * 8 * 8 * 3 - 1), dict(width=70000, height=70000)):
        assert call(**kw) == -1, kw


def test_wrappers_declare_the_recorded_spaces_and_set_agent_pov():
    """Host-side only: the facade's wrappers on a stand-in env (the engine behind the real one needs a GPU)."""
    from twoarmy_amd.gym_minigrid import wrappers as wr
    from twoarmy_amd.gym_minigrid.minigrid import _Space
    z = pr.load_golden()
    ts_env, V, hl = (int(v) for v in z["wr_env"])
    env = types.SimpleNamespace(width=17, height=17, tile_size=ts_env, agent_view_size=V, highlight=bool(hl), agent_pov=False,
                                _eng=types.SimpleNamespace(device="cpu"), observation_space={"image": _Space(shape=(V, V, 3))})
    full = wr.RGBImgObsWrapper(env)
    assert full.observation_space["image"].shape == tuple(int(v) for v in z["wr_full_space"]) == (136, 136, 3)
    assert full.tile_size == 8 and full.highlight is True and env.highlight is False and env.tile_size == 17
    assert [bool(v) for v in z["wr_agent_pov"]] == [False, True] and env.agent_pov is False
    part = wr.RGBImgPartialObsWrapper(env)
    assert env.agent_pov is True and part.tile_size == 8
    assert part.observation_space["image"].shape == tuple(int(v) for v in z["wr_partial_space"]) == (56, 56, 3)
    # the quirk the recording pins: the returned images are the ENV's size (tile_size 17), not the declared one
    assert z["wr_full"].shape == (4, 17 * ts_env, 17 * ts_env, 3) and z["wr_partial"].shape == (4, V * ts_env, V * ts_env, 3)
