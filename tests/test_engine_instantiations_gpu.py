"""Every kernel instantiation a launch of the engine can select -- PIPE_KERNELS[VARIANT][LAYOUT][PG] (24) and
ROLLOUT_KERNELS[E][VARIANT][FAST] (12) -- run once with the selection pinned through last_launch() and every output
compared bit-exactly with the CPU oracle, at the smallest sizes that reach them: selection boundaries, ragged last
groups, the XCD remap of the workgroup index, the second ring chunk and the grid stride of the fallback launch.
DESIGN.md ("engine instantiations") maps each table entry to its test id here."""
import numpy as np
import pytest
import torch

import twoarmy_oracle as orc
from test_engine_gpu import SEED, _canon, _compare_rollout, _engine, _inject, _oracle, padded_rows

pytestmark = pytest.mark.gpu

KEYS = ("obs", "matrix", "pos", "reward", "terminated", "truncated")
MAT_PITCH, MATC_PITCH = 292, 304


def _ceil(a, b):
    return (a + b - 1) // b


def _error():
    from twoarmy_amd._lib import TwoarmyLibraryError
    return TwoarmyLibraryError


def _pg_of(N):
    """Envs per workgroup of the pipelined kernel: the smallest of 2, 4, 8, 16 that leaves at most 256 workgroups --
    except that one round of 16-env workgroups (up to 4096 envs) becomes two rounds of 8-env ones."""
    pg = next((g for g in (2, 4, 8) if _ceil(N, g) <= 256), 16)
    return 8 if pg == 16 and _ceil(N, 16) <= 256 else pg


def _pipe(N, layout, T, epw=0):
    E = epw or (2 if N >= 2048 else 1)
    pg = _pg_of(N)
    return dict(pipelined=1, PG=pg, LAYOUT=layout, pipe_grid=_ceil(N, pg), E=E, FAST=int(layout != 2),
                seq_grid=min(_ceil(N, E), 256), T=T)


def _seq(N, E, fast, T):
    return dict(pipelined=0, PG=0, LAYOUT=0, pipe_grid=0, E=E, FAST=fast, seq_grid=_ceil(N, E), T=T)


def _obs_pitch(view):
    return (view * view * 3 + 15) // 16 * 16


def _raw_rows(out, view, nlead=2):
    """The padded native rows behind obs and matrix, pad included."""
    codes = out["matrix"].dtype == torch.uint8
    return (padded_rows(out["obs"], nlead, _obs_pitch(view)),
            padded_rows(out["matrix"], nlead, MATC_PITCH if codes else MAT_PITCH))


def _pad_hooks(view, layout_suffix=None):
    """before / after hooks of _compare_rollout: fill every native row, pad included, before the launches; afterwards
    the pad bytes / floats behind the image and the matrix must be zero (the kernels write whole 16-byte chunks)."""
    def before(eng, out):
        if layout_suffix is not None:
            assert out["matrix"]._tw_layout.endswith(layout_suffix), out["matrix"]._tw_layout
        o, m = _raw_rows(out, view)
        o.fill_(0xAB)
        m.fill_(7)

    def after(eng, out):
        o, m = _raw_rows(out, view)
        assert o.shape[-1] == _obs_pitch(view) and m.shape[-1] in (MAT_PITCH, MATC_PITCH)
        if o.shape[-1] > view * view * 3:
            assert int(o[..., view * view * 3:].max()) == 0, "image pad"
        assert float(m[..., 289:].float().abs().max()) == 0.0, "matrix pad"
        assert eng.fallback_count() == 0
    return before, after


# ------------------------------------------------------------------ a. selection boundaries
@pytest.mark.parametrize("N,pg", [(512, 2), (513, 4), (1024, 4), (1025, 8), (4096, 8), (4097, 16)])
def test_pg_boundaries(N, pg):
    """Envs per workgroup double where ceil(N / PG) would pass 256 workgroups; 4096 envs stay at 8 (two rounds of 512)."""
    want = _pipe(N, 1, 8)
    assert want["PG"] == pg and want["pipe_grid"] == _ceil(N, pg)
    _compare_rollout(6, N, 8, 17, supply_actions=True, expect=want)


def _philox_draws(N, T, env0=0):
    """The eight draw words the engine would take from Philox, as explicit draws [T, N, 8]."""
    lib = orc.lib()
    w = np.array([[[lib.tw_oracle_draw_word(SEED, env0 + n, t, s) for s in range(8)] for n in range(N)] for t in range(T)],
                 np.uint32)
    return torch.from_numpy(w.view(np.int32)).cuda()


SELECTION = {   # name: (T, keyword arguments of _compare_rollout, the launch they must select at N = 130)
    "T7-sequential": (7, dict(supply_actions=True), _seq(130, 1, 1, 7)),
    "T8-pipelined-slab-L1": (8, dict(supply_actions=True), _pipe(130, 1, 8)),
    "noslab-L0": (8, dict(supply_actions=True, slab=False), _pipe(130, 0, 8)),
    "codes-slab-L2": (8, dict(supply_actions=True, codes=True), _pipe(130, 2, 8)),
    "codes-noslab-L2": (8, dict(supply_actions=True, codes=True, slab=False), _pipe(130, 2, 8)),
    "dense": (8, dict(supply_actions=True, dense=True), _seq(130, 1, 0, 8)),
    "actions-None": (8, dict(), _seq(130, 1, 0, 8)),
    "draws": (8, dict(supply_actions=True, draws=True), _seq(130, 1, 0, 8)),
    "no-autoreset": (8, dict(supply_actions=True, autoreset=False), _seq(130, 1, 1, 8)),
}


@pytest.mark.parametrize("name", list(SELECTION))
def test_selection_conditions(name):
    """PIPE_MIN_T = 8, and what keeps a launch off the pipelined kernel: no auto-reset, dense rows, in-kernel actions,
    explicit draws.  The frame layout follows from the pointers: slab -> records, two allocations -> two streams, a
    uint8 matrix -> code frames from either allocator."""
    T, kw, want = SELECTION[name]
    kw = dict(kw)
    if kw.get("draws"):
        kw["draws"] = _philox_draws(130, T)
    _compare_rollout(4, 130, T, 17, expect=want, **kw)


# ------------------------------------------------------------------ b. the pipelined table
PIPE_N = [   # (PG, N, T, env0, second allocator for code frames)
    (2, 3, 130, 5, False), (2, 511, 130, 0, True),                  # 511, 1021, 2041, 4210: grid % 8 == 0, XCD remap
    (4, 513, 130, 1 << 20, True), (4, 1021, 130, 0, False),
    (8, 1025, 130, 77, False), (8, 2041, 130, 0, True),
    (16, 4210, 12, 12345, False), (16, 4097, 130, 0, True)]        # 4097 x 130 carries the ring wrap of PG = 16
PIPE_CASES = [pytest.param(v, pg, N, T, env0, layout, slab, id="v%d-PG%d-N%d-L%d-%s" % (v, pg, N, layout, "slab" if slab else "torch"))
              for v in (6, 4) for pg, N, T, env0, both in PIPE_N
              for layout, slab in [(0, False), (1, True), (2, True)] + ([(2, False)] if both else [])]


@pytest.mark.parametrize("variant,pg,N,T,env0,layout,slab", PIPE_CASES)
def test_pipelined_table(variant, pg, N, T, env0, layout, slab):
    """PIPE_KERNELS[variant][layout][pg], each with a ragged last workgroup, with and without the XCD remap of the
    workgroup index, through the second ring chunk (T = 130 = 128 + 2; two staging items per thread at PG = 16) and
    several auto-resets.  No fallback, and the pad of every native row is zero."""
    want = _pipe(N, layout, T)
    assert want["PG"] == pg and want["pipe_grid"] == {3: 2, 511: 256, 513: 129, 1021: 256, 1025: 129, 2041: 256,
                                                      4097: 257, 4210: 264}[N]
    before, after = _pad_hooks(17)
    _compare_rollout(variant, N, T, 17, env0=env0, supply_actions=True, codes=layout == 2, slab=slab, expect=want,
                     before=before, after=after)


# d. chunked hand-over in LAYOUT 0 (placed here: its 4097-env case shares the oracle run of the table's last cases)
@pytest.mark.parametrize("N,chunk", [(4097, [129, 1]), (513, 9)])
def test_pipelined_two_streams_chunked(N, chunk):
    """State carried from launch to launch through the ping-pong buffers; launches shorter than 8 steps (the last 4 of
    130 = 14 x 9 + 4, and the single step after 129) run the sequential kernel on what the pipelined one left."""
    def want(tlen):
        return _pipe(N, 0, tlen) if tlen >= 8 else _seq(N, 2 if N >= 2048 else 1, 1, tlen)
    before, after = _pad_hooks(17)
    _compare_rollout(4, N, 130, 17, chunk=chunk, supply_actions=True, slab=False, expect=want, before=before, after=after)


def test_pipelined_hipmalloc_slab():
    """The slab backed by plain hipMalloc memory (TW_F_SLAB_HIPMALLOC) asked for directly: same records, same kernel."""
    before, after = _pad_hooks(17, ", hipMalloc")
    _compare_rollout(6, 513, 130, 17, env0=1 << 20, supply_actions=True, slab="hipmalloc", expect=_pipe(513, 1, 130),
                     before=before, after=after)


# ------------------------------------------------------------------ c. view sizes
@pytest.mark.parametrize("view,layout", [(v, l) for v in (3, 5, 7, 9, 11, 13, 15) for l in (0, 1)])
def test_pipelined_views(view, layout):
    """Every view size below 17 in both float layouts: the per-lane emission constants of the two table rows
    (chunk = lane for two streams, lane - 9 for records)."""
    before, after = _pad_hooks(view)
    _compare_rollout(4, 513, 130, view, supply_actions=True, slab=layout == 1, expect=_pipe(513, layout, 130),
                     before=before, after=after)


@pytest.mark.parametrize("view,dense", [(11, False), (11, True), (13, False), (13, True)])
def test_sequential_views_11_13(view, dense):
    _compare_rollout(4, 513, 130, view, dense=dense, expect=_seq(513, 1, 0, 130))


@pytest.mark.parametrize("view", [11, 13])
def test_gen_obs_views_11_13(view):
    """tw_gen_obs at a view size other than the engine's, from the state 20 steps into an episode (no auto-reset, so
    the state is the one the last step's observation was made of)."""
    N, T = 130, 20
    eng = _engine(4, N, 17, seed=SEED)
    eng.rollout(T, eng.alloc_outputs(T), autoreset=False)
    ref = orc.rollout(4, N, T, SEED, view=view, autoreset=False)
    assert np.array_equal(eng.gen_obs(view).cpu().numpy(), ref["obs"][T - 1])
    eng.close()


# ------------------------------------------------------------------ e. the sequential table
SEQ_CASES = [pytest.param(v, N, epw, fast, id="v%d-N%d-E%d-FAST%d" % (v, N, epw, fast))
             for v in (6, 4) for N in (5, 130) for epw in (1, 2, 4) for fast in (1, 0)]     # N: E = 2, 4 leave a ragged last group


@pytest.mark.parametrize("variant,N,epw,fast", SEQ_CASES)
def test_sequential_table(variant, N, epw, fast):
    """ROLLOUT_KERNELS[epw][variant][fast]: FAST = 1 needs supplied actions and native rows (the slab), in-kernel
    actions give FAST = 0.  60 steps pass the 50-step cap."""
    _compare_rollout(variant, N, 60, 17, env0=3, epw=epw, pipeline=False, supply_actions=bool(fast),
                     expect=_seq(N, epw, fast, 60))


@pytest.mark.parametrize("variant,N,epw", [(v, N, epw) for v in (6, 4) for N in (5, 130) for epw in (2, 4)])
def test_sequential_fast_step_api(variant, N, epw):
    """The same FAST = 1 instantiations one tw_step at a time."""
    _compare_rollout(variant, N, 60, 17, env0=3, epw=epw, pipeline=False, supply_actions=True, step_api=True,
                     expect=_seq(N, epw, 1, 1))


def test_sequential_fast_without_autoreset():
    _compare_rollout(4, 130, 60, 17, env0=3, epw=2, supply_actions=True, autoreset=False, expect=_seq(130, 2, 1, 60))


# ------------------------------------------------------------------ f. the fallback launch with a grid stride
@pytest.mark.parametrize("N,epw,E,envs", [(300, 0, 1, (0, 270, 299)),         # 300 groups: a second pass for 44 workgroups
                                          (2050, 0, 2, (0, 1500, 2049)),      # 1025 groups: five passes
                                          (1100, 4, 4, (0, 1050, 1099))])     # 275 groups: two passes
@pytest.mark.parametrize("case", ["drift", "grid"])
def test_fallback_grid_stride(N, epw, E, envs, case):
    """A pipelined launch that meets an injected state is re-run by the sequential kernel behind it, which has at most
    256 workgroups and walks the env groups with a grid stride: outputs and final state equal a sequential engine's,
    with the injected envs in the first group, the last one and one that only a later pass reaches."""
    T = 40
    assert envs[1] // E >= 256 and envs[2] == N - 1 and _ceil(N, E) > 256
    a, b = _engine(6, N, 17, seed=SEED), _engine(6, N, 17, seed=SEED)
    for eng in (a, b):
        eng.set_envs_per_wave(epw)
        _inject(eng, case, envs)
    b.set_pipeline(False)
    acts = a.fill_actions(T)
    oa, ob = a.alloc_outputs(T), b.alloc_outputs(T)
    a.rollout(T, oa, actions=acts)
    b.rollout(T, ob, actions=acts)
    torch.cuda.synchronize()
    want = _pipe(N, 1, T, epw)
    assert want["seq_grid"] == 256 and want["pipelined"] == 1 and want["E"] == E
    assert a.last_launch() == want and b.last_launch() == _seq(N, E, 1, T)
    for k in KEYS:
        assert torch.equal(oa[k], ob[k]), k
    for x, y, name in zip(_canon(a.get_state()), _canon(b.get_state()), ("type", "colour", "records")):
        assert np.array_equal(x, y), name
    assert a.fallback_count() == 1 and b.fallback_count() == 0


# ------------------------------------------------------------------ g. rejections on the host
def test_rejected_calls_launch_nothing():
    """Arguments the library refuses before it launches anything: last_launch() keeps the launch before them and the
    engine goes on exactly where it was."""
    from twoarmy_amd import _lib
    from twoarmy_amd._marshal import ptr, stream
    N, T = 130, 8
    ref = _oracle(6, N, 2 * T, 17, 0)
    eng = _engine(6, N, 17, seed=SEED)
    acts = eng.fill_actions(2 * T)
    out = eng.alloc_outputs(2 * T)
    first = {k: v[:T] for k, v in out.items()}
    eng.rollout(T, first, actions=acts[:T])
    seen = eng.last_launch()
    assert seen == _pipe(N, 1, T)

    outs, flags = eng._out_args((T, N), first, 3)            # valid device pointers throughout
    assert outs[1] == 2048 and outs[3] == 512

    def rollout(T_, obs_pitch):
        a = list(outs)
        a[1] = obs_pitch
        _lib.check(_lib.lib().tw_rollout(eng._h, T_, ptr(acts[:T]), None, *a, flags, stream(eng.device)), "tw_rollout")

    for call in (lambda: eng.set_envs_per_wave(3), lambda: rollout(0, 2048), lambda: rollout(T, 17 * 17 * 3 - 1),
                 lambda: eng.gen_obs(4), lambda: eng.gen_obs(19)):
        with pytest.raises(_error()):
            call()
        assert eng.last_launch() == seen

    second = {k: v[T:] for k, v in out.items()}
    eng.rollout(T, second, actions=acts[T:])
    torch.cuda.synchronize()
    assert eng.last_launch() == seen and eng.fallback_count() == 0
    for k in KEYS:
        assert np.array_equal(out[k].cpu().numpy(), ref[k]), k
    eng.close()
