"""ppo_run_ends and ppo_gae_runs (csrc/ppo_kernels.hip): the run ends bit for bit against the numpy restatement, the scan
against the float64 statement of gae_runs_ref.py within the rounding bound derived there, its bit-exact special cases
against ppo_gae, the scan tree bit for bit at every structural edge on inputs whose float32 arithmetic is exact,
isolation of non-finite values at level 0 and through the upper levels, every argument rule, and the trainer's her_gae
path.  The two stream checks of both entry points are cases of the table in test_streams_gpu.py.  The sizes are the
smallest that reach every edge.  With float inputs: one record, a chunk of 64 less / exactly / plus one, 256 and 257, a
wavefront's 512 and a workgroup's 2048 less / exactly / plus one (2049: three launches), 1 000, 4 097, and 70 001 (35
workgroups).  With exact inputs (the boundary sweep): the same level-0 edges as array ends, 4096 and 4097, and level 1
and above: 64 * 2048 and one more (the second chunk of level 1), 512 * 2048 + 1 (its second wavefront), 2048^2 (a full
top level of two), 2048^2 + 1 and + 2049 (three levels, five launches; level 1 holds 2049 and 2050 maps, level 2
two) and 2048^2 + 512 * 2048 + 1 (513 maps behind the level-2 edge: the reduce of level 1 folds full chunks and two
wavefronts).  gae_runs_ref.LEVEL_EDGES is the table."""
import ctypes as C

import numpy as np
import pytest
import torch

import gae_runs_ref as gr
from gae_runs_ref import BLOCK, CHUNK, WAVE, _k, _records
from nav_util import Boxed
from ppo_util import DEV, accepted, dev as _dev, lib as _lib, lib_module as _libmod, ops as _ops, ptr as _P
from stream_util import host, same_bits

pytestmark = pytest.mark.gpu
EPS32 = gr.EPS32
PARAMS = [(0.99, 0.0), (0.99, 0.95), (1.0, 1.0)]
SIZES = [1, 63, 64, 65, 256, 257, 511, 512, 513, 1000, 2047, 2048, 2049, 4097, 70001]


# ------------------------------------------------------------------------------------------------ ppo_run_ends
def _at_end(a):
    """A device copy of `a` that ends where its 0xFF-filled buffer ends: what lies behind the last record is not ours."""
    a = np.ascontiguousarray(a)
    buf = torch.full((256 + a.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    t = buf[256:].view(torch.from_numpy(a).dtype).view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() + a.nbytes == buf.data_ptr() + buf.numel()
    return t


def _run_ends(t, n, goal, done, broken=None):
    return host(_ops().run_ends(_at_end(t), _at_end(n), _at_end(goal), _at_end(done), broken))


@pytest.mark.parametrize("H", [1, 2, 255, 256, 257, 70001])
def test_run_ends_equal_the_numpy_restatement(H):
    t, n, goal, done = _records(H, H)
    cases = [("as emitted", None, t, n, goal, done)]             # (name, run_end[j] if the case pins it, arrays)
    j = max(0, min(H - 2, H // 2))                                 # a record in mid-array, changed one way at a time
    if H > 1:
        done = done.copy()
        done[j] = 0
        t, n, goal = t.copy(), n.copy(), goal.copy()
        t[j + 1], n[j + 1], goal[j + 1] = t[j] + 1, n[j], goal[j]  # j -> j + 1 now links
        assert gr.run_ends(t, n, goal, done)[0][j] == 0
        for name, arr, val in (("n differs", n, n[j] + 1), ("t is not +1", t, t[j] + 2), ("t repeats", t, t[j])):
            a2 = arr.copy()
            a2[j + 1] = val
            cases.append((name, 1) + tuple(a2 if x is arr else x for x in (t, n, goal, done)))
        for k in (0, 1):
            g2 = goal.copy()
            g2[j + 1, k] += 1
            cases.append(("goal[%d] differs" % k, 1, t, n, g2, done))
        d2 = done.copy()
        d2[j] = 1
        cases.append(("done in mid-run", 1, t, n, goal, d2))
        g2 = goal.copy()
        g2[j] = g2[j + 1] = np.nan
        cases.append(("a NaN goal never links", 1, t, n, g2, done))
        g2 = goal.copy()
        g2[j], g2[j + 1] = (0.0, -0.0), (-0.0, 0.0)
        cases.append(("-0.0 links with +0.0", 0, t, n, g2, done))
    for name, end_at_j, ct, cn, cg, cd in cases:
        want, want_broken = gr.run_ends(ct, cn, cg, cd)
        assert end_at_j is None or want[j] == end_at_j, name
        broken = torch.full((1,), 1000, dtype=torch.int32, device=DEV)
        got = _run_ends(ct, cn, cg, cd, broken)
        assert got.dtype == np.uint8 and np.array_equal(got, want), name
        assert int(broken) == 1000 + want_broken, name              # added to, not overwritten
        assert np.array_equal(_run_ends(ct, cn, cg, cd, None), want), name       # NULL broken


def test_run_ends_never_reads_the_record_behind_the_last():
    """H records of H + 1: the record behind the last one would continue its run.  With the count H the last record ends
    its run, is counted as out of pattern, and run_end[H] keeps its sentinel."""
    for H in (1, 256, 1024, 1025):
        t = np.arange(H + 1, dtype=np.int32)
        n = np.full(H + 1, 3, np.int32)
        goal = np.full((H + 1, 2), 5, np.float32)
        done = np.zeros(H + 1, np.uint8)
        args = [_dev(x) for x in (t, n, goal, done)]
        run_end = torch.full((H + 1,), 0xAB, dtype=torch.uint8, device=DEV)
        broken = torch.zeros(1, dtype=torch.int32, device=DEV)
        assert accepted("ppo_run_ends", [_P(a) for a in args] + [C.c_int64(H), _P(run_end), _P(broken)])
        got = host(run_end)
        assert got[:H].tolist() == [0] * (H - 1) + [1] and got[H] == 0xAB and int(broken) == 1


def test_run_ends_rejections_launch_nothing():
    from test_ppo_kernels_edges_gpu import _each_rejected, _fill
    H = 5
    t, n, goal, done = (_dev(x) for x in _records(H, 1))
    outs = [_fill(H, torch.uint8, 77), _fill(1, torch.int32, 77)]
    good = [_P(t), _P(n), _P(goal), _P(done), C.c_int64(H), _P(outs[0]), _P(outs[1])]
    bad = [(i, None) for i in (0, 1, 2, 3, 5)] + [(4, C.c_int64(0)), (4, C.c_int64(-1)), (4, C.c_int64(1 << 40))]
    _each_rejected("ppo_run_ends", good, bad, outs, 77)


# ------------------------------------------------------------------------------------------------ ppo_gae_runs
def _gae_runs(r, v, nv, done, end, gamma, lam, mask, want_ret=True):
    out = _ops().gae_runs(_dev(r), _dev(v), _dev(nv), None if done is None else _dev(done), _dev(end), gamma, lam, mask,
                          want_ret=want_ret)
    return [None if x is None else host(x) for x in out]


def _patterns(H):
    return ["singletons", "runs64", "runs64+1", "her", "whole"] + (["one1000"] if H == 70001 else [])


@pytest.mark.parametrize("H", SIZES)
def test_gae_runs_vs_float64_reference(H):
    r, v, nv = gr.inputs(H, H)
    worst = 0.0
    for kind in _patterns(H):
        end = gr.pattern(kind, H, H)
        done = gr.dones(end, H)
        for (gamma, lam), mask in [(p, m) for p in PARAMS for m in (False, True)]:
            adv, tgt, ret = _gae_runs(r, v, nv, done if mask else None, end, gamma, lam, mask)
            assert all(np.isfinite(x).all() for x in (adv, tgt, ret))
            t32, d32 = gr.one_step32(r, v, nv, done, gamma, mask)
            assert same_bits(tgt, t32), (kind, gamma, lam, mask)
            if lam == 0.0 or kind == "singletons":               # the path the trainer uses today, bit for bit
                one = _ops().gae(*(_dev(x).view(1, H) for x in (r, v, nv)), _dev(done).view(1, H) if mask else None,
                                 gamma=gamma, lam=lam, use_done_mask=mask)
                for got, want in zip((adv, tgt, ret), one):
                    assert same_bits(got, host(want).reshape(-1)), (kind, gamma, lam, mask)
                assert same_bits(adv, d32) and same_bits(ret, d32 + v)
                continue
            a64, _, r64, S, L = gr.gae_runs64(r, v, nv, done, end, gamma, lam, mask)
            bound = _k(L, H) * EPS32 * S
            err = np.abs(adv - a64)
            ok = err <= bound
            worst = max(worst, float((err / np.where(bound > 0, bound, 1)).max()))
            assert ok.all(), "adv: %.3g x bound at %d (%s gamma %g lambda %g mask %d, L %d)" % (
                (err / bound)[~ok].max(), int(np.argmax(~ok)), kind, gamma, lam, mask, L[int(np.argmax(~ok))])
            # ret = fl(adv + v): the adv bound plus one rounding of |ret| <= S_j + |v|
            assert (np.abs(ret - r64) <= bound + EPS32 * (S + np.abs(v))).all(), (kind, gamma, lam, mask)
    print("H %d: worst err / bound %.3g" % (H, worst))


def test_gae_runs_twice_gives_equal_bits_and_nullable_outputs_change_nothing():
    H = 70001
    r, v, nv = gr.inputs(H, 9)
    end = gr.pattern("one1000", H, 9)
    done = gr.dones(end, 9)
    a = _gae_runs(r, v, nv, done, end, 0.99, 0.95, True)
    b = _gae_runs(r, v, nv, done, end, 0.99, 0.95, True)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    tr, tv, tnv, td, te = (_dev(x) for x in (r, v, nv, done, end))
    ws = torch.full((_lib().ppo_gae_runs_workspace(H),), np.nan, device=DEV)      # written before it is read
    for keep in ((0,), (1,), (2,), (0, 1), (1, 2), ()):
        outs = [torch.full((H,), np.nan, device=DEV) if i in keep else None for i in range(3)]
        args = [_P(x) for x in (tr, tv, tnv, td, te)] + [0.99, 0.95, 1, C.c_int64(H)] + [_P(o) for o in outs] + [_P(ws)]
        assert accepted("ppo_gae_runs", args)
        assert all(same_bits(host(outs[i]), a[i]) for i in keep), keep
    none = _gae_runs(r, v, nv, None, end, 0.99, 0.95, False, want_ret=False)      # NULL done without the mask, NULL ret
    assert none[2] is None and same_bits(none[0], _gae_runs(r, v, nv, done, end, 0.99, 0.95, False)[0])


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_gae_runs_nonfinite_delta_stays_in_its_run(bad):
    H = 5000                                                       # three workgroups
    r, v, nv = gr.inputs(H, 11)
    end = gr.pattern("her", H, 11)
    end[BLOCK - 40:BLOCK + 40] = 0                                 # one run across the first workgroup carry ...
    end[BLOCK - 41] = end[BLOCK + 39] = 1
    run = np.concatenate([[0], np.cumsum(end)[:-1]]).astype(np.int64)
    spots = [0, 63, 64, BLOCK - 1, BLOCK + 39, 2 * BLOCK, H - 1, 700]
    dirty = r.copy()
    dirty[spots] = bad
    hit = np.isin(run, run[spots])
    for mask in (False, True):
        done = gr.dones(end, 11, mid_run=0.0)
        clean = _gae_runs(r, v, nv, done, end, 0.99, 0.95, mask)
        got = _gae_runs(dirty, v, nv, done, end, 0.99, 0.95, mask)
        for g, c in zip(got, clean):
            assert same_bits(g[~hit], c[~hit]) and np.isfinite(c).all()
        first = np.array([np.nonzero(run == k)[0][0] for k in run[spots]])       # a run's first record sees all of it
        assert not np.isfinite(got[0][first]).any()
        got0 = _gae_runs(dirty, v, nv, done, end, 0.99, 0.0, mask)               # lambda = 0: every other RECORD
        clean0 = _gae_runs(r, v, nv, done, end, 0.99, 0.0, mask)
        other = np.ones(H, bool)
        other[spots] = False
        for g, c in zip(got0, clean0):
            assert same_bits(g[other], c[other])


# ------------------------------------------------------------------------------------------------ the boundary sweep
SWEEP = [511, 512, 513, 2047, 2048, 2049, 4096, 4097, CHUNK * BLOCK, CHUNK * BLOCK + 1, WAVE * BLOCK + 1, BLOCK * BLOCK,
         BLOCK * BLOCK + 1, BLOCK * BLOCK + 2049,
         BLOCK * BLOCK + WAVE * BLOCK + 1]        # 513 maps behind the level-2 edge: the reduce of level 1 folds 8 full
#                                                   chunks and 2 wavefronts under the long run that ends on the last record


def _boxed_call(dev_in, done, end, gamma, lam, mask, H):
    """ppo_gae_runs through the C entry: every output and a NaN-filled workspace of exactly the queried size inside
    0xA5-filled buffers -> (adv, target, ret) on the host; the borders of all four buffers are intact."""
    outs = [Boxed(H, torch.float32) for _ in range(3)]
    ws = Boxed(_lib().ppo_gae_runs_workspace(H), torch.float32)
    ws.view.fill_(np.nan)                                          # written before it is read
    td, te = _dev(done), _dev(end)
    args = [_P(x) for x in dev_in] + [_P(td) if mask else None, _P(te), gamma, lam, int(mask), C.c_int64(H)]
    assert accepted("ppo_gae_runs", args + [_P(o.view) for o in outs] + [_P(ws.view)])
    got = []
    for name, box in zip(("adv", "target", "ret", "workspace"), outs + [ws]):
        b = host(box.buf)
        assert (b[:box.lo] == 0xA5).all() and (b[box.hi:] == 0xA5).all(), "%s: a border was written" % name
        got.append(b[box.lo:box.hi].view(np.float32))
    return got[:3]


def _first_difference(got, want, placed):
    i = int(np.argmax(got.view(np.uint32) != want.view(np.uint32)))
    run = [p for p in placed if p[0] <= i <= p[1]]
    return "first at record %d (block %d, wavefront %d, chunk %d, lane %d)%s: got %r, want %r" % (
        i, i // BLOCK, i % BLOCK // WAVE, i % WAVE // CHUNK, i % CHUNK, " in the placed run %s" % (run[0],) if run else "",
        got[i], want[i])


@pytest.mark.parametrize("H", SWEEP)
@pytest.mark.parametrize("family", list(gr.FAMILIES))
def test_gae_runs_boundary_sweep(family, H):
    """Bit for bit against the exact reference, with a run ending on, beginning on, straddling and (c = 1) reaching far
    across EVERY edge of the tree below H (gae_runs_ref.boundary_runs), mask off and on with a done record on either side
    of each edge.  A difference is a finding about the kernels or the level loop of the host entry: the index of the
    first one names the edge."""
    gamma, lam = gr.FAMILIES[family]
    bounds = gr.boundaries(H)
    r, v, nv = gr.exact_inputs(family, H, H)
    dev_in = [_dev(x) for x in (r, v, nv)]
    for variant in gr.variants(family):
        end, placed = gr.boundary_runs(H, bounds, variant, family != "c1", H)
        done = gr.boundary_dones(end, bounds, variant, H)
        for mask in (False, True):
            a64, _, _ = gr.exact_runs(r, v, nv, done, end, gamma, lam, mask)       # asserts exactness before the launch
            want_adv = a64.astype(np.float32)
            want_tgt, _ = gr.one_step32(r, v, nv, done, gamma, mask)
            adv, tgt, ret = _boxed_call(dev_in, done, end, gamma, lam, mask, H)
            where = (family, H, variant, "mask" if mask else "no mask")
            assert same_bits(tgt, want_tgt), (where, "target", _first_difference(tgt, want_tgt, placed))
            assert same_bits(adv, want_adv), (where, "adv", _first_difference(adv, want_adv, placed))
            want_ret = want_adv + v                                    # exact here
            assert same_bits(ret, want_ret), (where, "ret", _first_difference(ret, want_ret, placed))


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_gae_runs_nonfinite_delta_stays_in_its_run_through_the_upper_levels(bad):
    """test_gae_runs_nonfinite_delta_stays_in_its_run one and two levels higher, device against device.  A non-finite
    delta reaches a map of level >= 1 only through the run that covers a workgroup's first record (that workgroup's
    composite d is the advantage of its first record).  So the run "just before" an edge B of level 1 / 2 is the one over
    the first record of the last workgroup before B (map B / 2048 - 1, the last of its chunk / wavefront / workgroup of
    level 1), the straddling run lies over B itself (map B / 2048, the first behind the edge), and the bad record sits
    behind the workgroup's first record in both."""
    H = BLOCK * BLOCK + 2049
    r, v, nv = gr.inputs(H, 13)
    end = gr.pattern("her", H, 13)
    spots = []
    for B in gr.LEVEL_EDGES[1]:
        for first in (B - BLOCK - 10, B - 10):                         # 20 records over a workgroup's first record
            end[first - 1] = end[first + 19] = 1
            end[first:first + 19] = 0
            spots.append(first + 13)
    run = np.concatenate([[0], np.cumsum(end)[:-1]]).astype(np.int64)
    dirty = r.copy()
    dirty[spots] = bad
    hit = np.isin(run, run[spots])
    assert hit.sum() == 20 * len(spots) == 120
    first = np.array(spots) - 13
    done = gr.dones(end, 13, mid_run=0.0)
    dev_clean, dev_dirty = [_dev(x) for x in (r, v, nv)], [_dev(x) for x in (dirty, v, nv)]
    for mask in (False, True):
        clean = _boxed_call(dev_clean, done, end, 0.99, 0.95, mask, H)
        got = _boxed_call(dev_dirty, done, end, 0.99, 0.95, mask, H)
        for name, g, c in zip(("adv", "target", "ret"), got, clean):
            assert np.isfinite(c).all()
            assert same_bits(g[~hit], c[~hit]), (name, mask, int(np.argmax((g != c) & ~hit)))
        assert not np.isfinite(got[0][first]).any() and not np.isfinite(got[2][first]).any()


def test_gae_runs_rejections_launch_nothing():
    from test_ppo_kernels_edges_gpu import _each_rejected, _fill
    H = 9
    r, v, nv = (_dev(x) for x in gr.inputs(H, 2))
    done, end = torch.zeros(H, dtype=torch.uint8, device=DEV), torch.ones(H, dtype=torch.uint8, device=DEV)
    outs = [_fill(H) for _ in range(3)]
    ws = _fill(2)
    good = [_P(r), _P(v), _P(nv), _P(done), _P(end), 0.99, 0.95, 1, C.c_int64(H)] + [_P(o) for o in outs] + [_P(ws)]
    bad = [(i, None) for i in (0, 1, 2, 3, 4, 12)]                 # (3, None): the mask without done
    bad += [(8, C.c_int64(0)), (8, C.c_int64(-3)), (8, C.c_int64(1 << 40))]
    _each_rejected("ppo_gae_runs", good, bad, outs)
    ws_of = _lib().ppo_gae_runs_workspace
    assert [ws_of(h) for h in (0, -1, 1 << 40)] == [-1, -1, -1]
    assert [ws_of(h) for h in (1, 2048, 2049, 70001, 2048 * 2048, 2048 * 2048 + 1)] == [
        2, 2, 4, 70, 4096, 2 * 2049 + 2 * 2]
    assert [ws_of(h) for h in (CHUNK * BLOCK + 1, WAVE * BLOCK + 1, BLOCK * BLOCK + 2049)] == [
        2 * 65, 2 * 513, 2 * 2050 + 2 * 2]
    with pytest.raises(_libmod().TwoarmyLibraryError):             # the front end raises what the C call returns
        _ops().gae_runs(r, v, nv, None, end, 0.99, 0.95, True)


# ------------------------------------------------------------------------------------------------ trainer
N_ENVS, T_STEPS, MB = 64, 64, 1024
ROLLOUT = N_ENVS * T_STEPS


@pytest.fixture(scope="module")
def her_runs():
    """One v6 trainer (64 envs, T = 64, max_steps = 50, seeded), one rollout, one relabelling; compute_targets() under
    each setting of (gae_lambda, use_done_mask, her_gae, records).  MIOpen's deterministic kernels: two passes of the
    critic over one batch must agree bit for bit."""
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(1)
        eng = TwoarmyEngine(6, N_ENVS, 17, seed=9981, max_steps=50)
        agent = PPO()
        agent.K_epochs = 1
        tr = VecPPOTrainer(agent, eng, rollout_steps=T_STEPS, minibatch=MB, value_chunk=2048)
        tr.collect(uniforms=torch.rand(T_STEPS, N_ENVS, generator=torch.Generator().manual_seed(40)).to(tr.device))
        h = tr.relabel()
        H = int(h["t"].numel())
        assert H > 0

        def targets(lam, mask, her_gae, records):
            agent.gae_lambda, agent.use_done_mask, tr.her_gae, tr.her = lam, mask, her_gae, records
            tr.her_targets = None
            adv, ct = tr.compute_targets()
            kept = None if tr.her_targets is None else {k: host(x) for k, x in tr.her_targets.items()}
            return dict(adv=host(adv), target=host(ct), broken=tr.her_out_of_pattern, kept=kept)

        perm = torch.randperm(H, generator=torch.Generator().manual_seed(3)).to(tr.device)
        shuffled = {k: (x[perm].contiguous() if k != "counts" else x) for k, x in h.items()}
        out = dict(tr=tr, h=h, H=H, gamma=agent.gamma, shuffled={k: host(x) for k, x in shuffled.items()}, records={k: host(x) for k, x in h.items()},
                   one_step=targets(0.0, False, False, h), one_step_gae=targets(0.0, False, True, h),
                   rollout=targets(0.95, True, False, None), gae=targets(0.95, True, True, h),
                   gae_shuffled=targets(0.95, True, True, shuffled), one_step_shuffled=targets(0.0, False, False, shuffled))
        agent.gae_lambda, agent.use_done_mask, tr.her_gae, tr.her = 0.95, True, True, h
        yield out
        eng.close()
    finally:
        torch.backends.cudnn.deterministic = was


def test_her_gae_at_lambda_zero_is_the_default_path_bit_for_bit(her_runs):
    a, b = her_runs["one_step"], her_runs["one_step_gae"]
    assert a["adv"].shape == (ROLLOUT + her_runs["H"],) and a["kept"] is None and b["kept"] is not None
    assert same_bits(a["adv"], b["adv"]) and same_bits(a["target"], b["target"])
    assert a["broken"] == b["broken"] == 0


def test_her_gae_records_against_the_float64_reference(her_runs):
    g, ro, rec, H = her_runs["gae"], her_runs["rollout"], her_runs["records"], her_runs["H"]
    assert same_bits(g["adv"][:ROLLOUT], ro["adv"]) and same_bits(g["target"][:ROLLOUT], ro["target"])
    kept = g["kept"]
    end, broken = gr.run_ends(rec["t"], rec["n"], rec["goal"], rec["done"])
    assert same_bits(kept["run_end"], end) and broken == g["broken"] == 0
    assert np.array_equal(end, (rec["done"] != 0).astype(np.uint8))               # ppo_her_relabel's pattern
    a64, _, r64, S, L = gr.gae_runs64(rec["reward"], kept["value"], kept["next_value"], rec["done"], end, her_runs["gamma"], 0.95, True)
    assert L.max() > 1 and L.max() <= 50
    adv, ct = g["adv"][ROLLOUT:], g["target"][ROLLOUT:]
    bound = _k(L, H) * EPS32 * S
    print("H %d, longest run %d, worst err / bound %.3g" % (H, L.max(), (np.abs(adv - a64) / bound).max()))
    assert (np.abs(adv - a64) <= bound).all()
    assert same_bits(ct, adv + kept["value"])                                      # the critic target is ret = adv + V(s)
    assert np.abs(adv - her_runs["one_step_gae"]["adv"][ROLLOUT:]).max() > 1e-4    # and not the one-step advantage


def test_her_gae_records_out_of_pattern_get_their_own_delta(her_runs):
    g, rec = her_runs["gae_shuffled"], her_runs["shuffled"]
    kept = g["kept"]
    end, broken = gr.run_ends(rec["t"], rec["n"], rec["goal"], rec["done"])
    assert g["broken"] == broken > 0 and same_bits(kept["run_end"], end)
    assert g["broken"] == her_runs["one_step_shuffled"]["broken"]                  # the torch compare chain counts the same
    lone = (rec["done"] == 0) & (end != 0)
    _, d32 = gr.one_step32(rec["reward"], kept["value"], kept["next_value"], rec["done"], her_runs["gamma"], True)
    assert lone.sum() == broken and same_bits(g["adv"][ROLLOUT:][lone], d32[lone])
    assert np.isfinite(g["adv"]).all() and np.isfinite(g["target"]).all()


def test_without_her_gae_the_assertion_still_fires_and_update_trains_with_it(her_runs):
    tr, h, H = her_runs["tr"], her_runs["h"], her_runs["H"]
    tr.her_gae = False
    with pytest.raises(AssertionError, match="TD\\(0\\)"):
        tr.compute_targets()
    tr.her_gae = True
    total = ROLLOUT + H                                             # whole minibatches only, as test_stack_gpu does
    la, lv = tr.update(permutations=[torch.randperm(total)[:total // MB * MB]])
    assert np.isfinite(float(la)) and np.isfinite(float(lv)) and tr.her is None
