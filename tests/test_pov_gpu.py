"""mg_render_pov (include/minigrid_render.h) and everything built on it, on the GPU, byte for byte: every frame recorded
from the reference's get_pov_render (tests/golden/pov.npz), random worlds against the numpy restatement
(tests/pov_ref.py, itself pinned to the recording by tests/test_pov_cpu.py), the unaligned paths of the gather it shares
with mg_render inside guarded buffers, env_index and the error codes, the "rgb" / "rgb_partial" observations of
TwoarmyVecEnv over the recorded scripts, the facade's pixel wrappers, and mg_render itself against render.npz.

The recorded occlusion worlds hold lava, which this renderer does not draw: a frame that shows lava must report error 1
and equal the recording outside the lava tiles (102 of 480 frames); the rest must equal it whole (see test_pov_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import pov_ref as pr
import render_ref as rr

pytestmark = pytest.mark.gpu
SEED = 9981
VIEWS = ((3, 8), (7, 8), (3, 1), (3, 3))


def _mr():
    from twoarmy_amd import minigrid_render
    return minigrid_render


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ------------------------------------------------------------------------------------------------ recorded frames
def test_recorded_world_frames_with_the_recorded_mask_and_with_the_mask_of_gen_obs():
    z = pr.load_golden()
    whole = 0
    for c in range(int(z["n_worlds"])):
        ty, co, st, W, H, ax, ay, carry = pr.world_planes(c)
        rep = lambda a: np.stack([a] * 4)                                                               # noqa: E731
        d = [_dev(rep(a)) for a in (ty, co, st)]
        agent = [_dev(np.full(4, ax, np.int32)), _dev(np.full(4, ay, np.int32)), _dev(np.arange(4, dtype=np.int32))]
        cr = _dev(rep(carry)) if carry[0] else None                                                   # carrying NULL = nothing
        for V, ts in VIEWS:
            vis, ref = z["w_vis_%02d_%d" % (c, V)], z["w_pov_%02d_%d_%d" % (c, V, ts)]
            a = (rep(ty), rep(co), rep(st), W, H, [ax] * 4, [ay] * 4, range(4), V, ts, rep(carry), vis)
            want, werr = pr.pov_frames(*a)
            skip = pr.undrawn_pixels(*a)
            for given in (_dev(vis), None):
                err = torch.full((4,), -7, dtype=torch.int32, device="cuda")
                got = _mr().render_pov(d[0], d[1], d[2], W, H, *agent, V, ts, carrying=cr, vis_mask=given, error=err,
                                       see_through_walls=False).cpu().numpy()
                assert np.array_equal(got, want), (c, V, ts, given is None)
                assert err.cpu().numpy().tolist() == werr.tolist()
                diff = (got != ref).any(axis=3)
                assert not (diff & ~skip).any(), (c, V, ts, given is None)
            whole += int((werr == 0).sum())
    assert whole == 378


@pytest.mark.parametrize("name", ["K4_goal", "K5_ball_onto_agent"])
def test_recorded_script_frames_with_null_mask_and_null_carrying(name):
    z, g = pr.load_golden(), rr.load_golden()
    V, ts = int(z["s_meta_" + name][2]), int(z["s_meta_" + name][3])
    frames, agents, grids = pr.load_script(name), z["s_agents_" + name], g["grids_" + name]
    p = np.ascontiguousarray(np.transpose(grids, (0, 2, 1, 3))).reshape(len(grids), 289, 3)
    err = torch.full((len(frames),), -7, dtype=torch.int32, device="cuda")
    got = _mr().render_pov(_dev(p[..., 0]), _dev(p[..., 1]), None, 17, 17, _dev(agents[:, 0]), _dev(agents[:, 1]),
                           _dev(agents[:, 2]), V, ts, error=err)
    assert got.shape == (len(frames), V * ts, V * ts, 3) and np.array_equal(got.cpu().numpy(), frames)
    assert not err.any()


# ------------------------------------------------------------------------------------------------ random worlds
def _random_worlds(W, H, N, seed):
    """Every drawable object, doors in three states; agents on every corner and edge, one step outside on each side
    and at random cells, in every direction; carried objects for a third of the envs."""
    rs = np.random.RandomState(seed)
    combos = [(0, 0, 0), (1, 0, 0)] * 6 + [(t, c, 0) for t in (2, 3, 5, 6, 7, 8) for c in range(6)] + \
             [(4, c, s) for c in range(6) for s in range(3)]
    pick = rs.randint(len(combos), size=(N, W * H))
    cells = np.array(combos, np.uint8)[pick]
    spots = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2),
             (-1, 1), (W, H - 2), (2, -1), (W - 2, H), (-1, -1), (W, H)]
    ax, ay, ad = (np.zeros(N, np.int32) for _ in range(3))
    for e in range(N):
        k = e + seed
        ax[e], ay[e] = spots[(k // 4) % len(spots)] if e < 4 * len(spots) else (rs.randint(W), rs.randint(H))
        ad[e] = k % 4
    carry = np.zeros((N, 3), np.uint8)
    for e in range(0, N, 3):
        carry[e] = combos[12 + rs.randint(len(combos) - 12)]
    return cells[..., 0].copy(), cells[..., 1].copy(), cells[..., 2].copy(), ax, ay, ad, carry


@pytest.mark.parametrize("ts", [1, 3, 8, 17])
@pytest.mark.parametrize("W,H", [(5, 4), (17, 17)])
def test_random_worlds_equal_restatement(W, H, ts):
    for N in (1, 5, 67):
        for V in (1, 2, 3, 7):
            ty, co, st, ax, ay, ad, carry = _random_worlds(W, H, N, 10 * V + ts)
            vis = (np.random.RandomState(V + N).randint(0, 4, (N, V, V)) != 0).astype(np.uint8)
            d = [_dev(a) for a in (ty, co, st, ax, ay, ad)]
            for v, c, s in ((vis, carry, st), (None, None, None)):           # every nullable pointer given, then NULL
                err = torch.full((N,), -7, dtype=torch.int32, device="cuda")
                got = _mr().render_pov(d[0], d[1], _dev(s), W, H, d[3], d[4], d[5], V, ts, carrying=_dev(c),
                                       vis_mask=_dev(v), error=err)
                want, werr = pr.pov_frames(ty, co, s, W, H, ax, ay, ad, V, ts, c, v)
                assert got.shape == (N, V * ts, V * ts, 3)
                assert np.array_equal(got.cpu().numpy(), want), (N, V, v is None)
                assert err.cpu().numpy().tolist() == werr.tolist() == [0] * N


# ------------------------------------------------------------------------------------------------ ABI edges
def _raw_pov(ty, co, st, N, W, H, ax, ay, ad, stride, carry, idx, n_out, vis, V, ts, frame_ptr, pitch, err):
    from twoarmy_amd import _lib
    atlas = _mr().TileAtlas.get(ts, "cuda:0")

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())
    return _lib.lib().mg_render_pov(p(ty), p(co), p(st), N, W, H, p(ax), p(ay), p(ad), stride, p(carry), p(idx), n_out,
                                    p(vis), V, p(atlas.tiles), ts, C.c_void_p(frame_ptr), pitch, p(err),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("V,ts", [(3, 3), (7, 8), (2, 1), (7, 17)])
def test_unaligned_frames_and_pitches_inside_guarded_buffers(V, ts):
    """Frame bases 0..3 bytes off alignment x dense and five pitches: exactly the frame's bytes are written.  (2, 1) is
    a frame shorter than one 16-byte chunk; (7, 17) takes more than one workgroup per frame."""
    N, W, H = 3, 6, 5
    ty, co, st, ax, ay, ad, carry = _random_worlds(W, H, N, 7)
    ref, _ = pr.pov_frames(ty, co, st, W, H, ax, ay, ad, V, ts, carry, None)
    F = V * V * ts * ts * 3
    d = [_dev(a) for a in (ty, co, st, ax, ay, ad, carry)]
    for base in range(4):
        for pitch in (0, F + 1, F + 2, F + 3, F + 13, F + 64):
            P = pitch or F
            buf = torch.full((64 + base + N * P + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            rc = _raw_pov(d[0], d[1], d[2], N, W, H, d[3], d[4], d[5], 1, d[6], None, N, None, V, ts,
                          buf.data_ptr() + 64 + base, pitch, None)
            assert rc == 0
            got = buf.cpu().numpy()
            want = np.full_like(got, 0xA5)
            for e in range(N):
                want[64 + base + e * P:64 + base + e * P + F] = ref[e].reshape(-1)
            assert np.array_equal(got, want), (base, pitch, int((got != want).sum()))


def test_env_index_error_codes_and_record_strided_agents():
    from twoarmy_amd._lib import TW_REC_WORDS
    W, H, V, ts, N = 9, 7, 5, 4, 6
    ty, co, st, ax, ay, ad, carry = _random_worlds(W, H, N, 3)
    ax[:], ay[:], ad[:] = 4, 3, np.arange(N) % 4                # everything within two cells of (4, 3) is in view
    carry[:] = 0
    ty[2, 3 * W + 3] = 9                                        # lava in front of the agent of world 2 (it faces left)
    ty[4, 2 * W + 4], co[4, 2 * W + 4] = 2, 6                   # a wall of colour 6 next to the agent of world 4
    carry[5] = (9, 0, 0)                                        # world 5 carries what is not drawn
    rec = np.full((N, TW_REC_WORDS), -12345, np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2] = ax, ay, ad
    rec_d = _dev(rec)
    ref, rerr = pr.pov_frames(ty, co, st, W, H, ax, ay, ad, V, ts, carry, None)
    assert rerr.tolist() == [0, 0, 1, 0, 1, 1]
    d = [_dev(a) for a in (ty, co, st, carry)]
    idx = np.array([5, 4, 2, 2, 0, 9, -1, 0], np.int32)        # reversed, with repeats; 9 and -1 are outside 0..N-1
    F = V * V * ts * ts * 3
    frame = torch.full((len(idx), F), 0x5A, dtype=torch.uint8, device="cuda")
    err = torch.full((len(idx),), -7, dtype=torch.int32, device="cuda")
    base = rec_d.data_ptr()

    class _At:                                                 # the three columns of the records, as raw addresses
        def __init__(self, off):
            self.off = off

        def data_ptr(self):
            return base + 4 * self.off
    rc = _raw_pov(d[0], d[1], d[2], N, W, H, _At(0), _At(1), _At(2), TW_REC_WORDS, d[3], _dev(idx), len(idx), None, V, ts,
                  frame.data_ptr(), 0, err)
    assert rc == 0
    got = frame.cpu().numpy()
    assert err.cpu().numpy().tolist() == [1, 1, 1, 1, 0, 2, 2, 0]
    for o, e in enumerate(idx):
        if 0 <= e < N:
            assert np.array_equal(got[o], ref[e].reshape(-1)), o
        else:
            assert (got[o] == 0x5A).all(), o                   # a frame with a bad index is left untouched
    # the lava cell of world 2 is somewhere in its view, drawn as the lit empty tile
    cells = pr.view_cells(ty[2], co[2], st[2], W, H, 4, 3, int(ad[2]), V)
    (j, i), = np.argwhere(cells[..., 0] == 9)
    tile = got[2].reshape(V * ts, V * ts, 3)[j * ts:(j + 1) * ts, i * ts:(i + 1) * ts]
    assert np.array_equal(tile, rr.render_tile(1, 0, 0, -1, 1, ts))


def test_argument_rejection_launches_nothing():
    W, H, V, ts, N = 6, 5, 3, 4, 2
    ty, co, st, ax, ay, ad, carry = _random_worlds(W, H, N, 5)
    d = [_dev(a) for a in (ty, co, st, ax, ay, ad)]
    F = V * V * ts * ts * 3
    frame = torch.full((N, F), 0x11, dtype=torch.uint8, device="cuda")
    ok = dict(ty=d[0], co=d[1], st=d[2], N=N, W=W, H=H, ax=d[3], ay=d[4], ad=d[5], stride=1, carry=None, idx=None, n_out=N,
              vis=None, V=V, ts=ts, frame_ptr=frame.data_ptr(), pitch=0, err=None)
    for kw in (dict(ty=None), dict(co=None), dict(ax=None), dict(ay=None), dict(ad=None), dict(frame_ptr=None), dict(N=0),
               dict(W=0), dict(H=0), dict(stride=0), dict(n_out=0), dict(n_out=N + 1), dict(V=0), dict(V=32),
               dict(pitch=F - 1), dict(pitch=1)):
        assert _raw_pov(**dict(ok, **kw)) == -1, kw
    torch.cuda.synchronize()
    assert (frame == 0x11).all()
    assert _raw_pov(**ok) == 0
    torch.cuda.synchronize()
    assert not (frame == 0x11).all()


# ------------------------------------------------------------------------------------------------ vector env
def _script(kind, name):
    """(recorded frames, ops, done flags, V, tile size): "rgb" replays render.npz, "rgb_partial" pov.npz."""
    z = pr.load_golden()
    ops, done = z["s_ops_" + name], z["s_done_" + name]
    if kind == "rgb":
        assert np.array_equal(ops, rr.load_golden()["ops_" + name])
        return rr.load_frames(name), ops, done, 17, 17
    return pr.load_script(name), ops, done, 7, 8


@pytest.mark.parametrize("name", ["K4_goal", "K5_ball_onto_agent"])
@pytest.mark.parametrize("kind", ["rgb", "rgb_partial"])
def test_vec_env_replays_the_recorded_frames(kind, name):
    """Without auto-reset the vector env is the recorded env: every frame, the done steps and the steps the script
    takes on the finished episode included.  2 envs; env 0 carries the recorded env id."""
    from twoarmy_amd.vecenv import TwoarmyVecEnv
    frames, ops, done, V, ts = _script(kind, name)
    eid = int(pr.load_golden()["s_meta_" + name][1])
    env = TwoarmyVecEnv(6, num_envs=2, agent_view_size=V, tile_size=ts, env_id0=eid, policy_actions=False, autoreset=False,
                        observation=kind)
    try:
        side = (17 if kind == "rgb" else V) * ts
        assert env.single_observation_shape == (side, side, 3)
        obs = env.reset()
        assert obs.dtype == torch.uint8 and obs.shape == (2, side, side, 3) and np.array_equal(obs[0].cpu().numpy(), frames[0])
        for k, op in enumerate(ops):
            if op == -1:
                obs = env.reset()
            else:
                obs, _, term, trunc, info = env.step(torch.full((2,), int(op), dtype=torch.int32))
                assert (int(term[0]), int(trunc[0])) == tuple(int(v) for v in done[k]), k
                assert "final_observation" not in info
            assert np.array_equal(obs[0].cpu().numpy(), frames[k + 1]), "%s op#%d=%d" % (name, k, op)
        assert np.array_equal((env.render_pov([0]) if kind == "rgb_partial" else env.render([0]))[0].cpu().numpy(), frames[-1])
    finally:
        env.close()


@pytest.mark.parametrize("name", ["K4_goal", "K5_ball_onto_agent"])
@pytest.mark.parametrize("kind", ["rgb", "rgb_partial"])
def test_vec_env_under_autoreset_shows_the_terminal_frame_then_the_next_episode(kind, name):
    """With auto-reset the done step returns the recorded terminal frame as final_observation and the recorded reset
    frame as observation; the steps after it are the reference's after a reset() that follows the done step at once
    (a_* of pov.npz: the scripts themselves step the finished episode a few more times first, and that moves state
    which outlives reset()).  K4 ends terminated, K5 truncated."""
    from twoarmy_amd.vecenv import TwoarmyVecEnv
    z = pr.load_golden()
    frames, ops, done, V, ts = _script(kind, name)
    after = np.bitwise_xor.accumulate(z[("a_full_" if kind == "rgb" else "a_pov_") + name], axis=0)
    tail = z["a_ops_" + name]
    eid = int(z["s_meta_" + name][1])
    first = int(np.argmax(done.any(axis=1)))
    assert tuple(done[first]) == ((1, 0) if name == "K4_goal" else (0, 1)) and len(after) == len(tail) + 1
    env = TwoarmyVecEnv(6, num_envs=2, agent_view_size=V, tile_size=ts, env_id0=eid, policy_actions=False, autoreset=True,
                        observation=kind)
    try:
        obs = env.reset()
        for k in range(first + 1):
            obs, _, term, trunc, info = env.step(torch.full((2,), int(ops[k]), dtype=torch.int32))
            assert (int(term[0]), int(trunc[0])) == tuple(int(v) for v in done[k]), k
            assert bool(info["_final_observation"][0]) == (k == first)
            assert np.array_equal(info["final_observation"][0].cpu().numpy(), frames[k + 1]), k
            assert np.array_equal(obs[0].cpu().numpy(), after[0] if k == first else frames[k + 1]), k
        for k, op in enumerate(tail):
            obs, _, term, trunc, info = env.step(torch.full((2,), int(op), dtype=torch.int32))
            assert not (bool(term[0]) or bool(trunc[0]) or bool(info["_final_observation"][0]))
            assert np.array_equal(info["final_observation"][0].cpu().numpy(), after[k + 1]), k
            assert np.array_equal(obs[0].cpu().numpy(), after[k + 1]), k
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ facade
def test_facade_wrappers_return_the_recorded_images():
    from twoarmy_amd.gym_minigrid import wrappers as wr
    from twoarmy_amd.gym_minigrid.envs.twoarmy import Twoarmy_v6
    z = pr.load_golden()
    ts_env, V, hl = (int(v) for v in z["wr_env"])
    env = Twoarmy_v6(agent_view_size=V, tile_size=ts_env, highlight=bool(hl), seed=SEED, env_id=0)
    try:
        full = wr.RGBImgObsWrapper(env)
        assert not env.agent_pov and np.array_equal(env.render(), z["wr_full"][0])
        part = wr.RGBImgPartialObsWrapper(env)
        assert env.agent_pov is True
        assert full.observation_space["image"].shape == tuple(z["wr_full_space"])
        assert part.observation_space["image"].shape == tuple(z["wr_partial_space"])
        for t in range(4):                                     # through the wrappers' own reset() / step()
            obs = full.step(int(z["wr_ops"][t - 1]))[0] if t else full.reset()
            f, p = obs["image"], part.observation(dict(obs))["image"]
            assert f.dtype == p.dtype == np.uint8 and obs["mission"] == env.mission
            assert np.array_equal(f, z["wr_full"][t]) and np.array_equal(p, z["wr_partial"][t]), t
            assert np.array_equal(env.get_pov_render(), p) and np.array_equal(env.render(), p)       # agent_pov is set
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ mg_render, unchanged
@pytest.mark.parametrize("name", ["K4_goal", "K5_ball_onto_agent_hl7"])
def test_mg_render_still_draws_the_recorded_frames(name):
    """The world instantiation of the shared gather, through mg_render, on the worlds behind the recorded full frames."""
    g = rr.load_golden()
    frames, grids, agents = rr.load_frames(name), g["grids_" + name], g["agents_" + name]
    hl, V = int(g["meta_" + name][3]), int(g["meta_" + name][4])
    p = np.ascontiguousarray(np.transpose(grids, (0, 2, 1, 3))).reshape(len(grids), 289, 3)
    a = [_dev(agents[:, k]) for k in range(3)]
    mask = _mr().highlight_mask(None, 17, 17, *a, V, n_envs=len(grids)) if hl else None
    got = _mr().render(_dev(p[..., 0]), _dev(p[..., 1]), _dev(p[..., 2]), 17, 17, *a, 17, highlight=mask)
    assert np.array_equal(got.cpu().numpy(), frames)
