"""Every instantiation and every ABI argument of the general MiniGrid view (csrc/minigrid_view.hip, C ABI in
include/minigrid_view.h) against oracle/minigrid_view_oracle.py, bit for bit (np.array_equal everywhere; these are
integer kernels and one double formula evaluated the way Python evaluates it).

  a  every compiled view size in both flavours (row-wise dword loads from 64 plane bytes on, byte per cell below)
  b  every runtime view size (1..31 minus the compiled ones)
  c  the agent on every border cell of a 5x4 world in every direction
  d  planes that start and end off 4-byte boundaries (the header's whole-word read contract)
  e  image_pitch and the destination phase (image base 0..3 bytes into a guarded buffer)
  f  vis_mask / state / carrying == NULL
  g  argument rejection before any launch
  h  mg_step: reward bits for every (step_count, max_steps <= 200), error / state == NULL, every border cell
  i  the Twoarmy engine's own view against the general kernel and the oracle in all four directions

The oracle itself is pinned to the reference's recorded images in test_minigrid_view_cpu.py (occlusion.npz for
V = 3..11, occlusion_wide.npz for 13, 15, 17, 21, 31); test_minigrid_view_edges_cpu.py pins COMPILED / MAX_VIEW below
to the dispatch switch of the source.  Oracle results are memoised per input, so the variants of one world (pitch,
alignment, NULL arguments) do not recompute them.

Conditions asserted on the inputs (they depend on the oracle alone): every occluded case of a-c has a hidden cell
and more visible cells than envs -- except V = 1, whose single cell is the agent's own and always visible, where
exactly N visible cells are required instead --; every batch of 8 or more envs holds all four directions, a carried
object and doors of all three states inside a window.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import minigrid_view_oracle as mvo

pytestmark = pytest.mark.gpu
DEV = "cuda"

COMPILED = (3, 5, 7, 9, 11, 13, 15, 17)            # case N: MG_LAUNCH_COLS(N) of mg_gen_obs
MAX_VIEW = 31                                      # MG_MAX_VIEW
RUNTIME = tuple(V for V in range(1, MAX_VIEW + 1) if V not in COMPILED)
ROWS_MIN_BYTES = 64                                # N * W * H from which the row-wise flavour is launched
TW_E_ARG = -1
TYPES = [1, 1, 1, 1, 2, 2, 4, 4, 5, 6, 7, 8, 9, 3]  # the object mix of test_view_kernel_matches_oracle_random
STEP_TYPES = [1, 1, 1, 2, 3, 4, 4, 5, 6, 7, 8, 8, 9, 11]

_BATCHES, _ORACLE, _DOORS = {}, {}, {}


class Batch:
    """N random worlds of W x H with one agent each; `key` identifies the content for the memo tables."""

    def __init__(self, key, enc, ax, ay, d, carry):
        self.key, self.enc, self.ax, self.ay, self.d, self.carry = key, enc, ax, ay, d, carry
        self.N, self.W, self.H = enc.shape[:3]


def batch(W, H, N, salt=0, agents=None):
    key = (W, H, N, salt, agents)
    if key in _BATCHES:
        return _BATCHES[key]
    rs = np.random.RandomState(W * 100003 + H * 1009 + N * 17 + salt)
    ty = rs.choice(TYPES, size=(N, W, H)).astype(np.uint8)
    co = rs.randint(0, 6, size=(N, W, H)).astype(np.uint8)
    st = np.where(ty == 4, rs.randint(0, 3, size=(N, W, H)), 0).astype(np.uint8)      # doors in all three states
    co[ty == 1] = 0
    if agents == "borders":                        # every (x, y, dir) of the world once
        assert N == W * H * 4
        ax, ay, d = (a.reshape(-1) for a in np.meshgrid(np.arange(W), np.arange(H), np.arange(4), indexing="ij"))
    else:                                          # anywhere inside the world, every direction present
        ax, ay, d = rs.randint(0, W, N), rs.randint(0, H, N), rs.permutation(np.arange(N) % 4)
    carry = np.zeros((N, 3), np.uint8)
    has = rs.rand(N) < 0.4
    if N >= 8 and not has.any():
        has[0] = True
    carry[has] = np.stack([rs.choice([5, 6, 7], has.sum()), rs.randint(0, 6, has.sum()), np.zeros(has.sum())], -1)
    b = _BATCHES[key] = Batch(key, np.stack([ty, co, st], -1), ax.astype(np.int64), ay.astype(np.int64),
                              d.astype(np.int64), carry)
    return b


def oracle(b, V, see_through, state=True, carrying=True):
    """Memoised mvo.gen_obs_batch; state=False / carrying=False = what a NULL argument must mean (all zeros)."""
    key = (b.key, V, bool(see_through), state, carrying)
    if key not in _ORACLE:
        enc = b.enc if state else b.enc * np.array([1, 1, 0], np.uint8)
        _ORACLE[key] = mvo.gen_obs_batch(enc, b.ax, b.ay, b.d, V, bool(see_through), b.carry if carrying else None)
    return _ORACLE[key]


def door_states_in_windows(b, V):
    key = (b.key, V)
    if key not in _DOORS:
        seen = set()
        for n in range(b.N):
            tx, ty = mvo.view_exts(int(b.ax[n]), int(b.ay[n]), int(b.d[n]), V)
            w = b.enc[n, max(tx, 0):max(tx + V, 0), max(ty, 0):max(ty + V, 0)].reshape(-1, 3)
            seen |= {int(s) for t, _, s in w if t == mvo.DOOR}
        _DOORS[key] = seen
    return _DOORS[key]


def flavour(b, V):
    if V not in COMPILED:
        return "runtime-V"
    return "rows" if b.N * b.W * b.H >= ROWS_MIN_BYTES else "bytes"


def honest(b, V, see_through):
    """Section "conditions" of the module docstring, from the oracle alone."""
    what = (V, flavour(b, V), b.W, b.H, b.N)
    if not see_through:
        vis = oracle(b, V, False)[1]
        if V == 1:
            assert int(vis.sum()) == b.N, what
        else:
            assert (vis == 0).any() and int(vis.sum()) > b.N, what
    if b.N >= 8:
        assert set(b.d.tolist()) == {0, 1, 2, 3} and (b.carry[:, 0] != 0).any(), what
        assert door_states_in_windows(b, V) == {0, 1, 2}, what


def same(got, want, b, V, what):
    """Exact equality; the message names V, flavour, world size, env index and the first differing cell."""
    if got.shape == want.shape and np.array_equal(got, want):
        return
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)[0]
    n = int(bad[0])
    raise AssertionError("%s: V=%d flavour=%s world %dx%d N=%d env %d (agent %d,%d dir %d) first differing cell %s: "
                         "got %d want %d (%d cells differ)" % (what, V, flavour(b, V), b.W, b.H, b.N, n, b.ax[n], b.ay[n],
                                                              b.d[n], tuple(int(v) for v in bad[1:]), got[tuple(bad)],
                                                              want[tuple(bad)], int((got != want).sum())))


def dev(a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def planes(b):
    from twoarmy_amd import minigrid_view as mv
    return tuple(p.to(DEV) for p in mv.planes_from_encoded(b.enc))


def run(b, V, see_through, state=True, carrying=True, want_mask=True, use_planes=None):
    from twoarmy_amd import minigrid_view as mv
    ty, co, st = use_planes if use_planes is not None else planes(b)
    img, vis = mv.gen_obs(ty, co, st if state else None, b.W, b.H, dev(b.ax, torch.int32), dev(b.ay, torch.int32),
                          dev(b.d, torch.int32), V, see_through, dev(b.carry) if carrying else None, want_mask)
    torch.cuda.synchronize()
    return img.cpu().numpy(), None if vis is None else vis.cpu().numpy()


def check(b, V, see_through):
    honest(b, V, see_through)
    want_img, want_vis = oracle(b, V, see_through)
    img, vis = run(b, V, see_through)
    same(vis, want_vis, b, V, "vis_mask")
    same(img, want_img, b, V, "image")


def n_partial(V):
    return 3 * (64 // V) + 1                       # three full wavefronts and one with a single env


# ------------------------------------------------------------------------------------------------ a: compiled sizes
ROWS_WORLDS = [(17, 17), (40, 5), (5, 40), (3, 3), (1, 9)]
BYTE_WORLDS = [(3, 3, 7), (7, 9, 1), (5, 4, 3), (1, 1, 63)]            # 63, 63, 60, 63 plane bytes
# seeds at which the one- and three-env batches meet the conditions of honest() at every compiled size (a 3x3 view
# hides a cell only behind an occluder right next to the agent) and hold a door and a carried object for the NULL tests
SALT = {(7, 9, 1): 148, (5, 4, 3): 1, (8, 8, 1): 94}


@pytest.mark.parametrize("see_through", [False, True])
@pytest.mark.parametrize("W,H", ROWS_WORLDS)
@pytest.mark.parametrize("V", COMPILED)
def test_compiled_sizes_rows_flavour(V, W, H, see_through):
    b = batch(W, H, n_partial(V))
    assert flavour(b, V) == "rows"
    check(b, V, see_through)


@pytest.mark.parametrize("see_through", [False, True])
@pytest.mark.parametrize("W,H,N", BYTE_WORLDS)
@pytest.mark.parametrize("V", COMPILED)
def test_compiled_sizes_byte_flavour(V, W, H, N, see_through):
    b = batch(W, H, N, SALT.get((W, H, N), 0))
    assert flavour(b, V) == "bytes" and N * W * H < ROWS_MIN_BYTES
    check(b, V, see_through)


@pytest.mark.parametrize("see_through", [False, True])
@pytest.mark.parametrize("V", COMPILED)
def test_flavour_threshold(V, see_through):
    """64 plane bytes take the row-wise kernel, 63 the byte-per-cell one."""
    at, below = batch(8, 8, 1, SALT.get((8, 8, 1), 0)), batch(7, 9, 1, SALT.get((7, 9, 1), 0))
    assert flavour(at, V) == "rows" and flavour(below, V) == "bytes"
    check(at, V, see_through)
    check(below, V, see_through)


# ------------------------------------------------------------------------------------------------- b: runtime sizes
def small_world(V):
    """A world smaller than the view (V = 1 has none: 1x1 is the view itself)."""
    return (1, 1) if V <= 2 else ((3, 3) if V % 2 == 0 or V < 10 else (1, 9))


@pytest.mark.parametrize("see_through", [False, True])
@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("V", RUNTIME)
def test_runtime_sizes(V, small, see_through):
    W, H = small_world(V) if small else (17, 17)
    assert not small or V == 1 or (W < V and (H < V or W == 1))
    b = batch(W, H, n_partial(V))
    assert flavour(b, V) == "runtime-V"
    check(b, V, see_through)


# ---------------------------------------------------------------------------------------------------- c: borders
@pytest.mark.parametrize("see_through", [False, True])
@pytest.mark.parametrize("V", COMPILED + (6, 16, 31))
def test_agent_on_every_border(V, see_through):
    b = batch(5, 4, 80, agents="borders")
    assert len({(x, y, d) for x, y, d in zip(b.ax, b.ay, b.d)}) == 80
    check(b, V, see_through)


# -------------------------------------------------------------------------------------------------- d: alignment
def embed(plane, off):
    """The plane bytes at address = off (mod 4) inside a 0xFF-filled tensor with >= 4 spare bytes on both sides."""
    n = plane.numel()
    buf = torch.full((((4 + off + n + 3) & ~3) + 4,), 0xFF, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0
    view = buf[4 + off:4 + off + n]
    view.copy_(plane.reshape(-1))
    assert view.data_ptr() % 4 == off and (view.data_ptr() + n) % 4 != 0 and buf.numel() - (4 + off + n) >= 4
    return buf, view.view(plane.shape)


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("W,H", [(17, 17), (3, 3)])
@pytest.mark.parametrize("V,N", [(3, 64), (7, 28), (13, 12), (17, 16)])
def test_unaligned_planes(V, N, W, H, shift):
    """The three planes 1, 2 and 3 bytes off a 4-byte boundary (`shift` rotates which plane gets which offset), their
    ends unaligned too (N*W*H is a multiple of 4), 0xFF -- no object type -- all around them."""
    b = batch(W, H, N)
    assert (N * W * H) % 4 == 0 and flavour(b, V) == "rows"
    emb = [embed(p, 1 + (k + shift) % 3) for k, p in enumerate(planes(b))]
    for see_through in (False, True):
        want_img, want_vis = oracle(b, V, see_through)
        img, vis = run(b, V, see_through, use_planes=[v for _, v in emb])
        same(vis, want_vis, b, V, "vis_mask (planes at offsets %s)" % [1 + (k + shift) % 3 for k in range(3)])
        same(img, want_img, b, V, "image (planes at offsets %s)" % [1 + (k + shift) % 3 for k in range(3)])
    for buf, v in emb:                                                  # the guard bytes are still there
        assert int((buf == 0xFF).sum().item()) >= buf.numel() - v.numel()


# ------------------------------------------------------------------------------------- e: image_pitch, image phase
def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t)


def abi_gen_obs(ty, co, st, N, W, H, ax, ay, d, carry, V, see_through, image, pitch, mask):
    from twoarmy_amd import _lib
    return _lib.lib().mg_gen_obs(ptr(ty), ptr(co), ptr(st), N, W, H, ptr(ax), ptr(ay), ptr(d), ptr(carry), V,
                                 int(see_through), ptr(image), pitch, ptr(mask),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("V", [4, 16, 3, 7, 13, 17])
def test_image_pitch_and_destination_phase(V):
    b = batch(17, 17, n_partial(V))
    ty, co, st = planes(b)
    ax, ay, d, carry = dev(b.ax, torch.int32), dev(b.ay, torch.int32), dev(b.d, torch.int32), dev(b.carry)
    want_img, want_vis = oracle(b, V, False)
    nb, N, lead = 3 * V * V, b.N, 16
    for pitch in sorted({nb, nb + 1, nb + 2, nb + 3, (nb + 15) & ~15, nb + 13}):
        for base in range(4):
            buf = torch.full((lead + base + N * pitch + 16,), 0xA5, dtype=torch.uint8, device=DEV)
            assert buf.data_ptr() % 4 == 0
            mask = torch.full((N, V, V), 0xA5, dtype=torch.uint8, device=DEV)
            rc = abi_gen_obs(ty, co, st, N, 17, 17, ax, ay, d, carry, V, False, buf.data_ptr() + lead + base, pitch, mask)
            torch.cuda.synchronize()
            assert rc == 0
            got = buf.cpu().numpy()
            rows = got[lead + base:lead + base + N * pitch].reshape(N, pitch)
            same(rows[:, :nb].reshape(N, V, V, 3), want_img, b, V, "image at pitch %d base %d" % (pitch, base))
            want = np.full(got.shape, 0xA5, np.uint8)
            want[lead + base:lead + base + N * pitch].reshape(N, pitch)[:, :nb] = want_img.reshape(N, nb)
            stray = np.flatnonzero(got != want)
            assert stray.size == 0, "V=%d pitch %d base %d: byte %d outside every image row was written (%d)" % (
                V, pitch, base, stray[0] - lead - base, got[stray[0]])
            same(mask.cpu().numpy(), want_vis, b, V, "vis_mask at pitch %d base %d" % (pitch, base))


# --------------------------------------------------------------------------------------------- f: nullable arguments
NULLABLE_CASES = [(7, 17, 17, None), (17, 17, 17, None), (6, 17, 17, None), (20, 17, 17, None), (7, 5, 4, 3), (13, 3, 3, 7)]


@pytest.mark.parametrize("V,W,H,N", NULLABLE_CASES)
def test_null_vis_mask_state_and_carrying(V, W, H, N):
    b = batch(W, H, N or n_partial(V), SALT.get((W, H, N), 0))
    assert (b.enc[..., 0] == mvo.DOOR).any() and (b.enc[..., 2] != 0).any() and (b.carry[:, 0] != 0).any()
    for see_through in (False, True):
        img, vis = run(b, V, see_through, want_mask=False)
        assert vis is None
        same(img, oracle(b, V, see_through)[0], b, V, "image with vis_mask = NULL")
        img, vis = run(b, V, see_through, state=False)
        same(vis, oracle(b, V, see_through, state=False)[1], b, V, "vis_mask with state = NULL")
        same(img, oracle(b, V, see_through, state=False)[0], b, V, "image with state = NULL")
        img, vis = run(b, V, see_through, carrying=False)
        same(vis, oracle(b, V, see_through, carrying=False)[1], b, V, "vis_mask with carrying = NULL")
        same(img, oracle(b, V, see_through, carrying=False)[0], b, V, "image with carrying = NULL")
    # a NULL state really changes what is expected here (closed doors open up), and so does NULL carrying
    assert not np.array_equal(oracle(b, V, False, state=False)[0], oracle(b, V, False)[0])
    assert not np.array_equal(oracle(b, V, False, carrying=False)[0], oracle(b, V, False)[0])


# ------------------------------------------------------------------------------------------------------ g: rejection
def test_gen_obs_rejects_bad_arguments_before_launch():
    V, N, W, H = 7, 10, 5, 4
    b = batch(W, H, N)
    ty, co, st = planes(b)
    ax, ay, d, carry = dev(b.ax, torch.int32), dev(b.ay, torch.int32), dev(b.d, torch.int32), dev(b.carry)
    image = torch.full((N, 32 * 32 * 3), 0xA5, dtype=torch.uint8, device=DEV)
    mask = torch.full((N, 32 * 32), 0xA5, dtype=torch.uint8, device=DEV)
    good = dict(ty=ty, co=co, st=st, N=N, W=W, H=H, ax=ax, ay=ay, d=d, carry=carry, V=V, see_through=False, image=image,
                pitch=image.shape[1], mask=mask)
    bad = [dict(V=0), dict(V=32), dict(V=-1), dict(N=0), dict(N=-5), dict(W=0), dict(H=0), dict(pitch=3 * V * V - 1),
           dict(pitch=-1), dict(ty=None), dict(co=None), dict(ax=None), dict(ay=None), dict(d=None), dict(image=None)]
    for change in bad:
        assert abi_gen_obs(**dict(good, **change)) == TW_E_ARG, change
    torch.cuda.synchronize()
    assert bool((image == 0xA5).all()) and bool((mask == 0xA5).all())
    assert abi_gen_obs(**good) == 0                                     # the unchanged call is accepted
    torch.cuda.synchronize()
    same(image[:, :3 * V * V].cpu().numpy().reshape(N, V, V, 3), oracle(b, V, False)[0], b, V, "image")
    assert bool((image[:, 3 * V * V:] == 0xA5).all())


def abi_step(ty, st, N, W, H, a, ax, ay, d, sc, max_steps, r, te, tr, err):
    from twoarmy_amd import _lib
    return _lib.lib().mg_step(ptr(ty), ptr(st), N, W, H, ptr(a), ptr(ax), ptr(ay), ptr(d), ptr(sc), max_steps, ptr(r),
                              ptr(te), ptr(tr), ptr(err), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def step_args(b, a, sc):
    ty, _, st = planes(b)
    N = b.N
    return dict(ty=ty, st=st, N=N, W=b.W, H=b.H, a=dev(a, torch.int32), ax=dev(b.ax, torch.int32),
                ay=dev(b.ay, torch.int32), d=dev(b.d, torch.int32), sc=dev(sc, torch.int32), max_steps=10,
                r=torch.full((N,), -7.0, dtype=torch.float64, device=DEV),
                te=torch.full((N,), 0xA5, dtype=torch.uint8, device=DEV),
                tr=torch.full((N,), 0xA5, dtype=torch.uint8, device=DEV),
                err=torch.full((N,), -7, dtype=torch.int32, device=DEV))


def test_step_rejects_bad_arguments_before_launch():
    b = batch(5, 4, 10)
    good = step_args(b, np.ones(b.N), np.zeros(b.N))
    bad = [dict(max_steps=0), dict(max_steps=-3), dict(N=0), dict(W=0), dict(H=0), dict(ty=None), dict(a=None),
           dict(ax=None), dict(ay=None), dict(d=None), dict(sc=None), dict(r=None), dict(te=None), dict(tr=None)]
    for change in bad:
        assert abi_step(**dict(good, **change)) == TW_E_ARG, change
    torch.cuda.synchronize()
    assert bool((good["r"] == -7.0).all()) and bool((good["te"] == 0xA5).all()) and bool((good["tr"] == 0xA5).all())
    assert bool((good["err"] == -7).all()) and bool((good["sc"] == 0).all())
    assert np.array_equal(good["ax"].cpu().numpy(), b.ax) and np.array_equal(good["ay"].cpu().numpy(), b.ay)
    assert abi_step(**good) == 0
    torch.cuda.synchronize()
    assert bool((good["sc"] == 1).all()) and bool((good["err"] >= 0).all())


# --------------------------------------------------------------------------------------------------------- h: mg_step
def test_step_reward_bits_for_every_step_count_and_max_steps():
    """reward == Python's 1 - 0.9 * ((step_count + 1) / max_steps) bit for bit for all 20 100 pairs
    0 <= step_count < max_steps <= 200 (a contracted fma(-0.9, q, 1) differs in 6 986 of them), truncated ==
    (step_count + 1 >= max_steps).  max_steps is one scalar per mg_step call, so the 20 100 envs go out as 200
    launches of max_steps envs each: an agent at (0, 1) facing right that steps right onto a goal at (1, 1)."""
    from twoarmy_amd import minigrid_view as mv
    enc1 = np.zeros((3, 3, 3), np.uint8)
    enc1[..., 0] = 1
    enc1[1, 1] = (8, 1, 0)
    world = mvo.Grid.from_encoded(enc1)
    total = truncs = 0
    for max_steps in range(1, 201):
        N = max_steps
        ty, _, st = (p.to(DEV) for p in mv.planes_from_encoded(np.repeat(enc1[None], N, 0)))
        sc0 = np.arange(N)
        ax, ay, sc = dev(np.zeros(N), torch.int32), dev(np.ones(N), torch.int32), dev(sc0, torch.int32)
        r, te, tr, err = mv.step(ty, st, 3, 3, dev(np.ones(N), torch.int32), ax, ay, dev(np.zeros(N), torch.int32), sc,
                                 max_steps)
        torch.cuda.synchronize()
        want_r = np.array([1 - 0.9 * ((s + 1) / max_steps) for s in range(N)], np.float64)
        want_tr = np.array([s + 1 >= max_steps for s in range(N)], np.uint8)
        for s in (0, N // 2, N - 1):                                    # the formula above is the oracle's
            assert mvo.step(world, 0, 1, 0, s, max_steps, 1) == (1, 1, s + 1, 0, True, bool(want_tr[s]), want_r[s])
        got_r = r.cpu().numpy()
        bad = np.flatnonzero(got_r.view(np.int64) != want_r.view(np.int64))
        assert bad.size == 0, "max_steps %d step_count %d: reward %s, Python gives %s (%d of %d differ)" % (
            max_steps, bad[0], float(got_r[bad[0]]).hex(), float(want_r[bad[0]]).hex(), bad.size, N)
        assert np.array_equal(tr.cpu().numpy(), want_tr), max_steps
        assert bool((te == 1).all()) and bool((err == 0).all()), max_steps
        assert np.array_equal(sc.cpu().numpy(), sc0 + 1) and bool((ax == 1).all()) and bool((ay == 1).all())
        total += N
        truncs += int(want_tr.sum())
    assert total == 20100 and truncs == 200


ACTIONS = [0, 1, 2, 3, 6, 4, 5, 7, -1]


def border_step_batch(W, H, max_steps):
    """The agent on every border cell x every direction x every action of ACTIONS, on random worlds."""
    cells = [(x, y) for x in range(W) for y in range(H) if x in (0, W - 1) or y in (0, H - 1)]
    combos = [(x, y, d, a) for (x, y) in cells for d in range(4) for a in ACTIONS]
    N = len(combos)
    rs = np.random.RandomState(W * 131 + H)
    ty = rs.choice(STEP_TYPES, size=(N, W, H)).astype(np.uint8)
    st = np.where(ty == 4, rs.randint(0, 3, size=(N, W, H)), 0).astype(np.uint8)
    enc = np.stack([ty, np.zeros_like(ty), st], -1)
    ax, ay, d, a = (np.array(v, np.int64) for v in zip(*combos))
    b = Batch(("step", W, H, max_steps), enc, ax, ay, d, np.zeros((N, 3), np.uint8))
    return b, a, rs.randint(0, max_steps + 2, N)


def step_oracle(b, a, sc, max_steps, state=True):
    enc = b.enc if state else b.enc * np.array([1, 1, 0], np.uint8)
    return np.array([mvo.step(mvo.Grid.from_encoded(enc[n]), int(b.ax[n]), int(b.ay[n]), int(b.d[n]), int(sc[n]),
                              max_steps, int(a[n])) for n in range(b.N)], np.float64)


@pytest.mark.parametrize("null_state", [False, True])
@pytest.mark.parametrize("null_error", [False, True])
@pytest.mark.parametrize("W,H", [(5, 3), (2, 6)])
def test_step_on_every_border_with_null_error_and_state(W, H, null_error, null_state):
    max_steps = 10
    b, a, sc = border_step_batch(W, H, max_steps)
    want = step_oracle(b, a, sc, max_steps, state=not null_state)
    # both exception kinds, a termination and a truncation occur, and a NULL state matters (a closed door is entered)
    assert (want[:, 3] == 1).any() and (want[:, 3] == 2).any() and (want[:, 4] == 1).any() and (want[:, 5] == 1).any()
    assert not np.array_equal(step_oracle(b, a, sc, max_steps, True), step_oracle(b, a, sc, max_steps, False))
    assert np.array_equal(want[:, 2], sc + 1)                           # step_count advances in every env, errors included
    g = step_args(b, a, sc)
    g["max_steps"] = max_steps
    if null_state:
        g["st"] = None
    err = g["err"]
    if null_error:
        g["err"] = None
    assert abi_step(**g) == 0
    torch.cuda.synchronize()
    got = np.stack([g[k].cpu().numpy().astype(np.float64) for k in ("ax", "ay", "sc")]
                   + [want[:, 3] if null_error else err.cpu().numpy().astype(np.float64)]
                   + [g[k].cpu().numpy().astype(np.float64) for k in ("te", "tr", "r")], 1)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "world %dx%d env %d (agent %d,%d dir %d action %d step_count %d) column %d: got %r want %r" % (
        W, H, bad[0][0], b.ax[bad[0][0]], b.ay[bad[0][0]], b.d[bad[0][0]], a[bad[0][0]], sc[bad[0][0]], bad[0][1],
        got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(got[:, 6].view(np.int64), want[:, 6].view(np.int64))
    if null_error:
        assert bool((err == -7).all())                                  # the caller's other memory is not touched


# ------------------------------------------------------------------------------- i: the engine's view, all directions
def test_twoarmy_engine_view_agrees_with_general_kernel_in_every_direction():
    """tw_gen_obs (see-through) == mg_gen_obs on the engine's own planes == the oracle, after a 30-step rollout, with
    directions 0..3 written into the DIR field, for every odd view size from 3 to 17."""
    from twoarmy_amd import minigrid_view as mv
    from twoarmy_amd.engine import FIELDS, TwoarmyEngine
    N = 128
    eng = TwoarmyEngine(4, N, 17, seed=9981)
    out = eng.alloc_outputs(30, obs=False, matrix=False)
    eng.rollout(30, out)
    torch.cuda.synchronize()
    ty, co, rec = eng.get_state()
    rec = rec.copy()
    rec[:, FIELDS["DIR"]] = np.arange(N) % 4
    eng.set_state(records=rec)
    ax, ay, d = (rec[:, FIELDS[k]].astype(np.int64) for k in ("AX", "AY", "DIR"))
    assert len({(int(x), int(y)) for x, y in zip(ax, ay)}) > 4          # the rollout moved the agents apart
    # planes hold cell (x, y) at y * 17 + x; type 0 reads as empty (include/minigrid_view.h)
    t2 = np.where(ty == 0, 1, ty).reshape(N, 17, 17).transpose(0, 2, 1)
    enc = np.stack([t2, co.reshape(N, 17, 17).transpose(0, 2, 1), np.zeros_like(t2)], -1).astype(np.uint8)
    b = Batch(("engine",), enc, ax, ay, d, np.zeros((N, 3), np.uint8))
    for V in range(3, 18, 2):
        want = mvo.gen_obs_batch(enc, ax, ay, d, V, True, None)[0]
        own = eng.gen_obs(V).cpu().numpy()
        img, _ = mv.gen_obs(torch.tensor(ty, device=DEV), torch.tensor(co, device=DEV), None, 17, 17,
                            dev(ax, torch.int32), dev(ay, torch.int32), dev(d, torch.int32), V, True)
        torch.cuda.synchronize()
        same(img.cpu().numpy(), want, b, V, "mg_gen_obs on the engine's planes")
        same(own, want, b, V, "tw_gen_obs")
    eng.close()
