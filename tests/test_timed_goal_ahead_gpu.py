"""mg_nav_timed_goal_ahead on the device (include/minigrid_nav.h): the look-ahead labels of records that each name their own
goal in a world whose blockers move, bit for bit against timed_goal_ahead_ref.py (a queue BFS over (cell, phase) per record's
env and goal, then ahead_ref's frontier loop) on the worlds test_timed_goal_ahead_cpu.py vets, and against the kernels it must
agree with; through the torch front end, TwoarmyEngine and VecSoATrainer.  The entry's two stream checks (a side stream
behind a delay, capture and replay) are a case of the table in test_streams_gpu.py."""
import numpy as np
import pytest
import torch

import timed_goal_ahead_ref as taref
import timed_nav_ref as tref
from nav_util import Boxed, dev, host, u16_full
from stream_util import hip_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = tref.UNREACHABLE
LEFT, RIGHT, UP, DOWN, SAME = 23, 25, 17, 31, 24


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


@pytest.fixture(autouse=True)
def no_hip_error():
    yield
    torch.cuda.synchronize()
    assert hip_error() == 0


_DEVICE = {}


def on_device(c):
    """The world's planes, schedule and rollout on the device, uploaded once."""
    if id(c) not in _DEVICE:
        _DEVICE[id(c)] = dict(ty=dev(c["ty"]), st=dev(c["st"]), sched=dev(c["sched"].view(np.int32)), pos=dev(c["pos"]),
                              age=dev(c["age"]), init=dev(c["init"]))
    return _DEVICE[id(c)]


def h16(t):
    """A uint16 device tensor on the host."""
    return host(t.view(torch.int16)).view(np.uint16)


def i64_full(shape, byte=0xA5):
    """nav_util.u16_full's int64 twin."""
    n = int(np.prod(shape))
    return torch.full((8 * n,), byte, dtype=torch.uint8, device=DEV).view(torch.int64).view(shape)


def run(c, rec, steps, off=(0, 0), with_dist=True, pad=24):
    """mg_nav_timed_goal_ahead through the front end, the outputs at element offsets `off` (labels, distances) from a 16-byte
    boundary inside 0xA5-filled buffers; every element outside the first R must keep its sentinel.  -> host outputs (labels
    as uint64, distances None when not asked for)."""
    d = on_device(c)
    R = len(rec["t"])
    la, ld = i64_full(off[0] + R + pad), u16_full(off[1] + R + pad)
    assert la.data_ptr() % 16 == 0 and ld.data_ptr() % 16 == 0
    out = la.view(torch.uint8)[8 * off[0]:8 * (off[0] + R)].view(torch.int64)
    dist_out = ld.view(torch.uint8)[2 * off[1]:2 * (off[1] + R)].view(torch.uint16)
    got = nav().timed_goal_ahead(d["ty"], dev(rec["t"]), dev(rec["n"]), dev(rec["goal"]), d["pos"], c["W"], c["H"], d["sched"],
                                 d["age"], d["init"], steps=steps, pass_types=c["pass_types"], state=d["st"], out=out,
                                 dist_out=dist_out if with_dist else False)
    assert got[0] is out and (got[1] is dist_out if with_dist else got[1] is None)
    ha, hd = host(la.view(torch.uint8)).reshape(-1, 8), host(ld.view(torch.uint8)).reshape(-1, 2)
    keep_a, keep_d = np.ones(len(ha), bool), np.ones(len(hd), bool)
    keep_a[off[0]:off[0] + R] = False
    if with_dist:
        keep_d[off[1]:off[1] + R] = False
    assert (ha[keep_a] == 0xA5).all() and (hd[keep_d] == 0xA5).all(), "an element outside the first R lost its sentinel"
    return host(out).view(np.uint64), h16(dist_out) if with_dist else None


def check(got, want, where):
    assert np.array_equal(got[0], want[0]), (where, np.flatnonzero(got[0] != want[0])[:8])
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), (where, np.flatnonzero(got[1] != want[1])[:8])


# ------------------------------------------------------------------------------------------------ the three worlds
@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("P", [1, 2, 16])
def test_small_world_equals_the_reference(P, steps):
    c = taref.small(P)
    assert nav().timed_goal_ahead_floods(5, 4, P) == 8
    check(run(c, c["rec"], steps), taref.want(c, steps), (P, steps))
    check(run(c, c["rec"], steps, off=(1, 3), with_dist=False), taref.want(c, steps), (P, steps, "no distances"))


@pytest.mark.parametrize("steps", [1, 2, 3])
def test_twoarmy_world_equals_the_reference_in_any_order_at_every_alignment(steps):
    """R = 2100: three workgroups, a run across either boundary.  `ahead` at a 16-byte aligned address and 8 bytes above
    one, acting_dist 2 bytes above one; the records in emission order and in one fixed permutation."""
    c = taref.twoarmy()
    rec, want = c["rec"], taref.want(c, steps)
    assert nav().timed_goal_ahead_floods(17, 17, 6) == 8 and len(rec["t"]) == 2100
    got = run(c, rec, steps, off=(0, 1))
    check(got, want, "aligned")
    check(run(c, rec, steps, off=(1, 1)), want, "ahead + 8 bytes")
    check(run(c, rec, steps, off=(1, 0), with_dist=False), want, "no distances")
    perm = np.random.default_rng(17).permutation(len(rec["t"]))
    again = run(c, {k: v[perm] for k, v in rec.items()}, steps, off=(0, 1))
    assert np.array_equal(again[0], got[0][perm]) and np.array_equal(again[1], got[1][perm])
    assert np.array_equal(got[0] != 0, got[1] != U)                                       # invariant (d)


@pytest.mark.parametrize("steps", [1, 3])
def test_large_world_floods_one_image_at_a_time(steps):
    c = taref.large()
    assert nav().timed_goal_ahead_floods(32, 32, 16) == 1
    check(run(c, c["rec"], steps, off=(1, 5)), taref.want(c, steps), steps)
    check(run(c, c["rec"], steps, with_dist=False), taref.want(c, steps), steps)


def test_no_records_launch_nothing():
    c = taref.twoarmy()
    d = on_device(c)
    e32, ef = torch.empty(0, dtype=torch.int32, device=DEV), torch.empty((0, 2), dtype=torch.float32, device=DEV)
    lab, ad = nav().timed_goal_ahead(d["ty"], e32, e32, ef, d["pos"], 17, 17, d["sched"], d["age"], d["init"],
                                     pass_types=c["pass_types"])
    assert lab.shape == (0,) and lab.dtype == torch.int64 and ad.shape == (0,) and ad.dtype == torch.uint16
    box = Boxed(0, torch.int64)
    assert nav().timed_goal_ahead(d["ty"], e32, e32, ef, d["pos"], 17, 17, d["sched"], d["age"], d["init"], out=box.view,
                                  dist_out=False)[1] is None and box.untouched()


# ------------------------------------------------------------------------------------------------ the invariants, kernel to kernel
@pytest.mark.parametrize("name", ["5x4 P=2", "17x17 Twoarmy", "32x32 P=16"])
def test_one_goal_per_env_equals_timed_field_then_ahead(name):
    """Invariant (a): mg_nav_timed_field from the goal, then mg_nav_ahead with that period."""
    c = taref.worlds()[name]
    d = on_device(c)
    W, H, N, T = c["W"], c["H"], c["N"], c["T"]
    gc = np.array([c["pool"][n][0] for n in range(N)])
    gx, gy = (gc % W).astype(np.int32), (gc // W).astype(np.int32)
    field = nav().timed_field(d["ty"], d["st"], W, H, d["sched"], c["pass_types"], goal=(dev(gx), dev(gy)))[0]
    order = np.random.default_rng(2).permutation(T * N)
    order = order[np.argsort(order % N, kind="stable")]               # runs of one env, steps in any order
    t, n = (order // N).astype(np.int32), (order % N).astype(np.int32)
    rec = dict(t=t, n=n, goal=np.stack([gy[n] + 0.5, gx[n] + 0.25], 1).astype(np.float32))
    for steps in (1, 2, 3):
        lab, ad = nav().ahead(field, d["pos"], W, H, steps=steps, age=d["age"], init_pos=d["init"])
        got = run(c, rec, steps)
        assert np.array_equal(got[0], host(lab).view(np.uint64)[t, n]) and np.array_equal(got[1], h16(ad)[t, n])
        assert (got[0] != 0).any()


@pytest.mark.parametrize("name", ["5x4 P=1", "17x17 Twoarmy", "32x32 P=16"])
def test_period_one_with_an_empty_schedule_equals_goal_ahead(name):
    """Invariant (b): mg_nav_goal_ahead on the same records."""
    c = taref.worlds()[name]
    d = on_device(c)
    W, H = c["W"], c["H"]
    rec = {k: dev(v) for k, v in c["rec"].items()}
    zero = torch.zeros((1, H), dtype=torch.int32, device=DEV)
    for steps in (1, 2, 3):
        want = nav().goal_ahead(d["ty"], rec["t"], rec["n"], rec["goal"], d["pos"], W, H, steps=steps,
                                pass_types=c["pass_types"], age=d["age"], init_pos=d["init"], state=d["st"])
        got = nav().timed_goal_ahead(d["ty"], rec["t"], rec["n"], rec["goal"], d["pos"], W, H, zero, d["age"], d["init"],
                                     steps=steps, pass_types=c["pass_types"], state=d["st"])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int16), want[1].view(torch.int16))
        assert bool((got[0] != 0).any())


@pytest.mark.parametrize("name", ["5x4 P=16", "17x17 Twoarmy", "32x32 P=16"])
def test_one_step_is_the_image_of_the_timed_move_set(name):
    """Invariant (c): mg_nav_timed_goal_moves on the same records, with the same acting_dist."""
    c = taref.worlds()[name]
    d = on_device(c)
    rec = c["rec"]
    m, ad = nav().timed_goal_moves(d["ty"], dev(rec["t"]), dev(rec["n"]), dev(rec["goal"]), d["pos"], c["W"], c["H"], d["sched"],
                                   d["age"], d["init"], c["pass_types"], state=d["st"])
    m = host(m).astype(np.uint64)
    image = sum(((m >> np.uint64(k)) & np.uint64(1)) << np.uint64(b) for k, b in enumerate((LEFT, RIGHT, UP, DOWN, SAME)))
    got = run(c, rec, 1)
    assert np.array_equal(got[0], image) and np.array_equal(got[1], h16(ad)) and (m & np.uint64(0x10)).any()


# ------------------------------------------------------------------------------------------------ engine and trainer
N_ENVS, T_STEPS = 8, 16


def _trainer(prior):
    from test_soa_cpu import seeded_agent
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.soa_vec import VecSoATrainer
    eng = TwoarmyEngine(6, N_ENVS, 17, seed=9981, max_steps=10)
    agent = seeded_agent()
    agent.K_epochs = agent.K_epochs_pre_agent_position = 1
    tr = VecSoATrainer(agent, eng, rollout_steps=T_STEPS, minibatch=64, value_chunk=512)
    assert tr.enable_orientation_prior(**prior)["hindsight_timed"] == prior.get("hindsight_timed", False)
    uni = torch.rand(T_STEPS + 1, N_ENVS, 3, generator=torch.Generator().manual_seed(40)).to(tr.device)
    tr.collect(uniforms=uni)
    tr.relabel()
    tr.term[:, ::2] |= tr.trunc[:, ::2]                              # the even envs "reach the goal" (test_orientation_prior_gpu)
    tr.label_ahead()
    return tr, eng


@pytest.mark.parametrize("timed_records", [True, False], ids=["hindsight_timed", "as before"])
def test_trainer_labels_its_hindsight_records_over_cell_and_phase(timed_records):
    import ahead_ref
    from twoarmy_amd.soa.soa_vec import VecSoATrainer
    with pytest.raises(ValueError, match="hindsight_timed=True needs hindsight=True"):
        VecSoATrainer.enable_orientation_prior(None, 0.5, timed=True, hindsight_timed=True)
    T, N = T_STEPS, N_ENVS
    sched = nav().twoarmy_schedule(blocks=True).numpy().astype(np.uint32)
    tr, eng = _trainer(dict(coef=0.5, timed=True, hindsight=True, hindsight_timed=timed_records))
    h = {k: host(tr.her[k]) for k in ("t", "n", "goal")}
    assert h["t"].size > 0 and tr._her_ahead_of is tr.her
    c = dict(W=17, H=17, N=N, T=T, P=6, ty=host(eng.plane_views()[0]), st=None, sched=sched, pass_types=taref.STATIC,
             pos=host(tr.pos[3:3 + T]), age=host(tr.age[:-1]), init=host(tr.init_pos), memo={})
    if timed_records:
        want = taref.timed_goal_ahead(c, h["t"], h["n"], h["goal"], 3)
    else:                                                              # as before: mg_nav_goal_ahead on the static map
        want = ahead_ref.goal_ahead(c["ty"], None, 17, 17, h["t"], h["n"], h["goal"], c["pos"], 3, c["age"], c["init"],
                                    pass_types=taref.STATIC)
        static = eng.goal_ahead(tr.her, tr.pos[3:3 + T], tr.age[:-1], tr.init_pos, pass_types=taref.STATIC)
        assert torch.equal(tr.her_ahead, static[0])
    assert np.array_equal(host(tr.her_ahead).view(np.uint64), want[0]) and np.array_equal(h16(tr.her_ahead_dist), want[1])
    assert (want[0] != 0).any()
    st = tr.orientation_prior_stats()
    assert set(st) == {"labelled", "agree", "her_labelled", "her_realised", "coef"} and st["her_labelled"] > 0
    torch.manual_seed(70)
    loss = tr.update_orientation()
    assert loss is not None and np.isfinite(float(loss)) and tr.orient_prior["updates"] == 1
    eng.close()
