"""The device renderer (include/minigrid_render.h) on the GPU, byte for byte: the atlas against every tile recorded
from the reference, the MiniGridEnv facade against every recorded frame, TwoarmyEngine.render and mg_render on worlds
built here against the numpy restatement (tests/render_ref.py, itself pinned to the recordings by
tests/test_render_cpu.py), the highlight mask against the recorded masks, and the ABI's edges: unaligned frame bases
and pitches inside guarded buffers, nullable pointers, record-strided agent arrays, unsupported cells, bad arguments."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_ref as rr
from golden_util import explicit_draws

pytestmark = pytest.mark.gpu
SEED = 9981


def _mr():
    from twoarmy_amd import minigrid_render
    return minigrid_render


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ------------------------------------------------------------------------------------------------ atlas
@pytest.mark.parametrize("ts", [8, 17, 32])
def test_atlas_equals_every_recorded_tile(ts):
    z = rr.load_golden()
    atlas = _mr().TileAtlas(ts, "cuda:0").tiles.cpu().numpy()
    assert atlas.shape == (rr.N_TILES, ts, ts, 3)
    bad = []
    for k, ref in zip(z["tilekeys_%d" % ts], z["tiles_%d" % ts]):
        k = [int(v) for v in k]
        if not np.array_equal(atlas[rr.tile_index(*k)], ref):
            bad.append((tuple(k), int((atlas[rr.tile_index(*k)] != ref).sum())))
    assert not bad, "tile_size %d: %d of %d tiles differ (key, bytes): %s" % (ts, len(bad), len(z["tiles_%d" % ts]), bad[:8])


@pytest.mark.parametrize("ts", [1, 2, 5, 11, 64])
def test_atlas_equals_restatement_at_unrecorded_sizes(ts):
    atlas = _mr().TileAtlas(ts, "cuda:0").tiles.cpu().numpy()
    for t in range(0, 9):
        for c in range(6):
            for s in (range(3) if t == rr.DOOR else (0,)):
                for a in range(-1, 4):
                    for h in (0, 1):
                        assert np.array_equal(atlas[rr.tile_index(t, c, s, a, h)], rr.render_tile(t, c, s, a, h, ts)), \
                            (ts, t, c, s, a, h)


# ------------------------------------------------------------------------------------------------ facade replay
@pytest.mark.parametrize("name", [str(n) for n in rr.load_golden()["script_names"]])
def test_facade_replays_every_recorded_frame(name):
    """get_full_render() after the constructor's reset and after every op of the script == the reference's frame: the
    wall drop in the frame of the step whose obs does not show it yet (K1), the goal and a ball under the agent
    (K4, K5), v4 patrols on the reference's own random stream (K8), the highlighted 7 x 7 view (K4 / K5 _hl7)."""
    from twoarmy_amd.gym_minigrid.envs.twoarmy import Twoarmy_v4, Twoarmy_v6
    z = rr.load_golden()
    variant, eid, natural, hl, V = (int(v) for v in z["meta_" + name])
    frames, ops = rr.load_frames(name), z["ops_" + name]
    nat = explicit_draws({"draw_log": z["draws_" + name]}) if natural else None
    env = (Twoarmy_v4 if variant == 4 else Twoarmy_v6)(agent_view_size=V, tile_size=17, highlight=bool(hl), seed=SEED,
                                                       env_id=eid)
    try:
        img = env.get_full_render()
        assert img.dtype == np.uint8 and img.shape == (289, 289, 3)
        assert np.array_equal(img, frames[0]), "%s reset frame: %d bytes differ" % (name, int((img != frames[0]).sum()))
        t = 0
        for k, op in enumerate(ops):
            if op == -1:
                env.reset()
            else:
                env.step(int(op), draws=nat.get(t, np.zeros(8, np.uint32)) if nat is not None else None)
                t += 1
            img = env.render()
            assert np.array_equal(img, frames[k + 1]), "%s op#%d=%d: %d bytes differ" % (
                name, k, op, int((img != frames[k + 1]).sum()))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ engine
def _engine_ref(eng, ts, highlight, rows):
    from twoarmy_amd._lib import FIELDS
    ty, co, rec = eng.get_state()
    ty, co, rec = ty[rows], co[rows], rec[rows]
    ax, ay, ad = rec[:, FIELDS["AX"]], rec[:, FIELDS["AY"]], rec[:, FIELDS["DIR"]]
    hm = None
    if highlight:
        hm = np.stack([rr.highlight_mask(None, 17, 17, int(x), int(y), int(d), eng.view_size) for x, y, d in zip(ax, ay, ad)])
    img, err = rr.render_frames(ty, co, None, 17, 17, ax, ay, ad, ts, hm)
    assert not err.any()
    return img


def test_engine_render_4096_envs_after_a_rollout():
    from twoarmy_amd.engine import TwoarmyEngine
    N, T = 4096, 64
    eng = TwoarmyEngine(4, N, 17, device="cuda:0", seed=SEED)
    try:
        out = eng.alloc_outputs(T)
        eng.rollout(T, out, actions=eng.fill_actions(T))
        frames = eng.render()                                            # all envs, tile_size 17
        assert frames.shape == (N, 289, 289, 3) and frames.dtype == torch.uint8
        again = torch.empty_like(frames)
        eng.render(out=again)
        assert torch.equal(frames, again)                                 # two launches, identical bytes
        del again
        for lo in range(0, N, 512):
            rows = np.arange(lo, lo + 512)
            assert np.array_equal(frames[lo:lo + 512].cpu().numpy(), _engine_ref(eng, 17, False, rows)), lo
        del frames
        idx = np.array([4095, 0, 77, 3000, 77, 1, 2048, 5, 4094], np.int32)        # non-monotonic, with a repeat
        sub = eng.render(env_index=_dev(idx), tile_size=17, highlight=True)
        assert np.array_equal(sub.cpu().numpy(), _engine_ref(eng, 17, True, idx))
        one = eng.render(env_index=_dev(idx[:1]), tile_size=8)
        assert np.array_equal(one.cpu().numpy(), _engine_ref(eng, 8, False, idx[:1]))
    finally:
        eng.close()


def test_vecenv_render():
    from twoarmy_amd.vecenv import TwoarmyVecEnv
    env = TwoarmyVecEnv("MiniGrid-twoarmy-17x17-v6", num_envs=64, agent_view_size=7, tile_size=8, highlight=True)
    try:
        env.reset()
        for t in range(20):
            env.step(torch.full((64,), (1, 2, 4)[t % 3], device=env.device))
        assert np.array_equal(env.render().cpu().numpy(), _engine_ref(env.engine, 8, True, np.arange(64)))
        assert np.array_equal(env.render([5, 3, 5]).cpu().numpy(), _engine_ref(env.engine, 8, True, np.array([5, 3, 5])))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ general worlds
def _object_world(W, H, N, seed):
    """N worlds of W x H cells that together hold every object of the set in every colour, doors in three states, empty
    cells of both codes; agents in every direction, standing on a goal, an open door, a floor cell, a ball, nothing."""
    rs = np.random.RandomState(seed)
    combos = [(0, 0, 0), (1, 0, 0)] + [(t, c, 0) for t in (2, 3, 5, 6, 7, 8) for c in range(6)] + \
             [(4, c, s) for c in range(6) for s in range(3)]
    assert W * H >= len(combos) + 8
    ty, co, st = (np.zeros((N, W * H), np.uint8) for _ in range(3))
    ax, ay, ad = (np.zeros(N, np.int32) for _ in range(3))
    stand = [(8, 1, 0), (4, 2, 0), (3, 4, 0), (6, 4, 0), (1, 0, 0)]
    for e in range(N):
        cells = combos + [combos[rs.randint(len(combos))] for _ in range(W * H - len(combos))]
        order = rs.permutation(W * H)
        for k, (t, c, s) in zip(order, cells):
            ty[e, k], co[e, k], st[e, k] = t, c, s
        want = stand[e % len(stand)]
        k = next(int(k) for k in range(W * H) if (ty[e, k], co[e, k], st[e, k]) == want)
        ax[e], ay[e], ad[e] = k % W, k // W, e % 4
    hl = (rs.randint(0, 3, (N, W * H)) == 0).astype(np.uint8)
    return ty, co, st, ax, ay, ad, hl


@pytest.mark.parametrize("ts", [8, 17, 32, 5])
@pytest.mark.parametrize("W,H", [(11, 7), (6, 13)])
def test_general_worlds_equal_restatement(ts, W, H):
    N = 10
    ty, co, st, ax, ay, ad, hl = _object_world(W, H, N, 100 + ts)
    err = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    got = _mr().render(_dev(ty), _dev(co), _dev(st), W, H, _dev(ax), _dev(ay), _dev(ad), ts, highlight=_dev(hl), error=err)
    ref, rerr = rr.render_frames(ty, co, st, W, H, ax, ay, ad, ts, hl)
    assert got.shape == (N, H * ts, W * ts, 3)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert err.cpu().numpy().tolist() == rerr.tolist() == [0] * N
    # NULL state = every door open; NULL highlight = none; an agent outside the world is not drawn
    ax2 = ax.copy()
    ax2[0], ax2[1] = -1, W
    got = _mr().render(_dev(ty), _dev(co), None, W, H, _dev(ax2), _dev(ay), _dev(ad), ts)
    ref, _ = rr.render_frames(ty, co, None, W, H, ax2, ay, ad, ts, None)
    assert np.array_equal(got.cpu().numpy(), ref)


@pytest.mark.parametrize("W,H,V", [(17, 17, 7), (9, 13, 3), (25, 6, 17), (5, 5, 31)])
def test_highlight_mask_equals_restatement(W, H, V):
    rs = np.random.RandomState(V)
    N = 64
    vis = (rs.randint(0, 4, (N, V, V)) != 0).astype(np.uint8)
    ax, ay = rs.randint(0, W, N).astype(np.int32), rs.randint(0, H, N).astype(np.int32)
    ad = (np.arange(N) % 4).astype(np.int32)
    got = _mr().highlight_mask(_dev(vis), W, H, _dev(ax), _dev(ay), _dev(ad), V).cpu().numpy()
    ref = np.stack([rr.highlight_mask(vis[e], W, H, int(ax[e]), int(ay[e]), int(ad[e]), V) for e in range(N)])
    assert np.array_equal(got, ref)
    got = _mr().highlight_mask(None, W, H, _dev(ax), _dev(ay), _dev(ad), V, n_envs=N).cpu().numpy()
    ref = np.stack([rr.highlight_mask(None, W, H, int(ax[e]), int(ay[e]), int(ad[e]), V) for e in range(N)])
    assert np.array_equal(got, ref)


def test_highlight_mask_equals_every_recorded_mask():
    """env.agent_coordinate of the reference on the 30 occlusion worlds x 4 directions x V in 3, 7, 17, from the
    reference's own visibility masks."""
    z = rr.load_golden()
    for c in range(int(z["n_mask_worlds"])):
        W, H, ax, ay = (int(v) for v in z["mask_meta_%02d" % c])
        for V in (3, 7, 17):
            vis, out = z["mask_vis_%02d_%d" % (c, V)], z["mask_out_%02d_%d" % (c, V)]
            got = _mr().highlight_mask(_dev(vis), W, H, _dev(np.full(4, ax, np.int32)), _dev(np.full(4, ay, np.int32)),
                                       _dev(np.arange(4, dtype=np.int32)), V).cpu().numpy()
            assert np.array_equal(got.reshape(4, H, W), out.transpose(0, 2, 1)), (c, V)


# ------------------------------------------------------------------------------------------------ ABI edges
def _raw_render(ty, co, st, N, W, H, ax, ay, ad, stride, idx, n_out, hl, ts, frame_ptr, pitch, err):
    from twoarmy_amd import _lib
    atlas = _mr().TileAtlas.get(ts, "cuda:0")

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())
    rc = _lib.lib().mg_render(p(ty), p(co), p(st), N, W, H, p(ax), p(ay), p(ad), stride, p(idx), n_out, p(hl),
                              p(atlas.tiles), ts, C.c_void_p(frame_ptr), pitch, p(err),
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc


@pytest.mark.parametrize("W,H,ts", [(6, 5, 7), (17, 17, 17), (3, 2, 1)])
def test_unaligned_frames_and_pitches_inside_guarded_buffers(W, H, ts):
    """Frame bases 0..3 bytes off alignment x dense and five pitches: exactly the frame's bytes are written."""
    N = 3
    ty, co, st, ax, ay, ad, hl = _object_world(17, 17, N, 7)
    ty, co, st, hl = (np.ascontiguousarray(a.reshape(N, 17, 17)[:, :H, :W].reshape(N, H * W)) for a in (ty, co, st, hl))
    ax, ay = (ax % W).astype(np.int32), (ay % H).astype(np.int32)
    ref, _ = rr.render_frames(ty, co, st, W, H, ax, ay, ad, ts, hl)
    F = H * W * ts * ts * 3
    d = [_dev(a) for a in (ty, co, st, ax, ay, ad, hl)]
    for base in range(4):
        for pitch in (0, F + 1, F + 2, F + 3, F + 13, F + 64):
            P = pitch or F
            buf = torch.full((64 + base + N * P + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            rc = _raw_render(d[0], d[1], d[2], N, W, H, d[3], d[4], d[5], 1, None, N, d[6], ts, buf.data_ptr() + 64 + base,
                             pitch, None)
            assert rc == 0
            got = buf.cpu().numpy()
            want = np.full_like(got, 0xA5)
            for e in range(N):
                want[64 + base + e * P:64 + base + e * P + F] = ref[e].reshape(-1)
            assert np.array_equal(got, want), (base, pitch, int((got != want).sum()))


def test_record_strided_agents_env_index_errors_and_single_frame():
    from twoarmy_amd._lib import TW_REC_WORDS
    W, H, ts, N = 11, 7, 5, 6
    ty, co, st, ax, ay, ad, hl = _object_world(W, H, N, 3)
    ty[2, 5], ty[4, 0], co[4, 1] = 9, 11, 6                   # lava; a subgoal and a wall of colour 6
    ty[4, 1] = 2
    rec = np.full((N, TW_REC_WORDS), -12345, np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2] = ax, ay, ad
    rec_d = _dev(rec)
    ref, rerr = rr.render_frames(ty, co, st, W, H, ax, ay, ad, ts, None)
    assert rerr.tolist() == [0, 0, 1, 0, 1, 0]
    d = [_dev(a) for a in (ty, co, st)]
    idx = np.array([4, 2, 0, 2, 9, -1, 5], np.int32)          # 9 and -1 are outside 0..N-1
    F = H * W * ts * ts * 3
    frame = torch.full((len(idx), F), 0x5A, dtype=torch.uint8, device="cuda")
    err = torch.full((len(idx),), -7, dtype=torch.int32, device="cuda")
    base = rec_d.data_ptr()

    class _At:                                                 # the three columns of the records, as raw addresses
        def __init__(self, off):
            self.off = off

        def data_ptr(self):
            return base + 4 * self.off
    rc = _raw_render(d[0], d[1], d[2], N, W, H, _At(0), _At(1), _At(2), TW_REC_WORDS, _dev(idx), len(idx), None, ts,
                     frame.data_ptr(), 0, err)
    assert rc == 0
    got = frame.cpu().numpy()
    assert err.cpu().numpy().tolist() == [1, 1, 0, 1, 2, 2, 0]
    for o, e in enumerate(idx):
        if 0 <= e < N:
            assert np.array_equal(got[o], ref[e].reshape(-1)), o
        else:
            assert (got[o] == 0x5A).all(), o                   # a frame with a bad index is left untouched
    # the lava cell of world 2 (cell (5, 0)) came out as an empty tile
    empty = rr.render_tile(1, 0, 0, int(ad[2]) if (ax[2], ay[2]) == (5, 0) else -1, 0, ts)
    assert np.array_equal(got[1].reshape(H * ts, W * ts, 3)[0:ts, 5 * ts:6 * ts], empty)
    # n_out = 1, error NULL, through the front end with a strided view of the records
    one = _mr().render(d[0], d[1], d[2], W, H, rec_d[:, 0], rec_d[:, 1], rec_d[:, 2], ts, env_index=_dev(idx[3:4]))
    assert np.array_equal(one.cpu().numpy()[0], ref[2])


def test_argument_rejection_on_the_device_path():
    from twoarmy_amd import _lib
    W, H, ts, N = 6, 5, 4, 2
    ty, co, st, ax, ay, ad, hl = _object_world(17, 17, N, 5)
    ty, co = (_dev(a[:, :W * H]) for a in (ty, co))
    ax, ay, ad = _dev((ax % W).astype(np.int32)), _dev((ay % H).astype(np.int32)), _dev(ad)
    atlas = _mr().TileAtlas.get(ts, "cuda:0").tiles
    F = H * W * ts * ts * 3
    frame = torch.full((N, F), 0x11, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                                          # noqa: E731
    ok = dict(type=p(ty), colour=p(co), state=None, n_envs=N, width=W, height=H, ax=p(ax), ay=p(ay), ad=p(ad), stride=1,
              env_index=None, n_out=N, highlight=None, atlas=p(atlas), ts=ts, frame=p(frame), pitch=0, error=None,
              stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for kw in (dict(type=None), dict(colour=None), dict(ax=None), dict(ay=None), dict(ad=None), dict(atlas=None),
               dict(frame=None), dict(n_envs=0), dict(width=0), dict(height=0), dict(stride=0), dict(n_out=0),
               dict(n_out=N + 1), dict(ts=0), dict(ts=257), dict(pitch=F - 1), dict(pitch=1)):
        a = dict(ok, **kw)
        assert _lib.lib().mg_render(*[a[k] for k in ok]) == -1, kw
    torch.cuda.synchronize()
    assert (frame == 0x11).all()                               # nothing was launched
    assert _lib.lib().mg_render(*ok.values()) == 0
    torch.cuda.synchronize()
    assert not (frame == 0x11).all()


def test_two_launches_give_identical_bytes():
    W, H, ts, N = 13, 9, 17, 32
    ty, co, st, ax, ay, ad, hl = _object_world(W, H, N, 9)
    d = [_dev(a) for a in (ty, co, st, ax, ay, ad, hl)]
    a = _mr().render(d[0], d[1], d[2], W, H, d[3], d[4], d[5], ts, highlight=d[6])
    b = _mr().render(d[0], d[1], d[2], W, H, d[3], d[4], d[5], ts, highlight=d[6])
    assert torch.equal(a, b)
    t1 = _mr().TileAtlas(ts, "cuda:0").tiles
    t2 = _mr().TileAtlas(ts, "cuda:0").tiles
    assert torch.equal(t1, t2)
