"""ppo_her_select (csrc/ppo_kernels.hip) bit for bit against tests/her_select_ref.py on the hand-built cases of that
module (70 steps x 5 envs: episodes across the 64-row chunk, of 1, 2, 64 and 65 records, around `skip`, with revisits,
+-0.0, positions outside the world, ties and unreachable keys), the records ppo_her_relabel makes of its choices, every
argument rule, the stream protocol of tests/stream_util.py, and VecPPOTrainer.relabel() under each rule over two
rollouts.  The stream cases live here; see the note at STREAM_CASES on test_streams_gpu.py's completeness check."""
import numpy as np
import pytest
import torch

import her_oracle
import her_select_ref as hs
import test_streams_gpu as streams
from her_select_ref import CASE_N, CASE_T, KEY16, LATE, SENTINEL, SIDE, TABLE
from ppo_util import DEV, dev as _d, lib as _lib, ops as _ops, ptr as _P, rejected, stream as _stream
from stream_util import Case, host, same_bits

pytestmark = pytest.mark.gpu
RULES = (LATE, KEY16, TABLE)
KEYS = ("counts", "t", "n", "goal", "reward", "done")
KW = dict(seed=11, env_id0=3, step0=100)


@pytest.fixture(scope="module")
def on_device():
    hs.check_cases_present()                                  # on the host, before anything is launched
    return {k: _d(np.array(v)) for k, v in hs.cases().items()}          # a copy: the shared arrays are read-only


def _select(b, rule, max_goals=4, skip=0, choices=None, stats=None, fill=SENTINEL, **kw):
    if choices is None:
        choices = torch.full((CASE_T, CASE_N, 4), fill, dtype=torch.int32, device=DEV)
    kw = {**KW, **kw}
    return _ops().her_select(b["pos"], b["terminated"], b["truncated"], b["age0"], rule, key16=b["key16"], table=b["table"],
                             width=SIDE, height=SIDE, max_goals=max_goals, skip=skip, choices=choices, stats=stats, **kw)


@pytest.mark.parametrize("rule", RULES)
def test_choices_and_stats_equal_the_restatement(on_device, rule):
    for skip in (0, 4):
        for max_goals in (1, 2, 3, 4):
            want_c, want_s, _ = hs.reference(rule, max_goals, skip)
            got_c, got_s = _select(on_device, rule, max_goals, skip)
            assert same_bits(host(got_c), want_c), (rule, max_goals, skip)
            assert same_bits(host(got_s), want_s), (rule, max_goals, skip, host(got_s), want_s)
    assert (want_c == SENTINEL).any() and (want_c >= 0).any()


def test_the_front_end_fills_its_own_choices_with_minus_one(on_device):
    b = on_device
    got_c, got_s = _ops().her_select(b["pos"], b["terminated"], b["truncated"], b["age0"], "late", **KW)
    want_c, want_s, _ = hs.run_case(LATE, fill=-1)
    assert same_bits(host(got_c), want_c) and same_bits(host(got_s), want_s)
    for name, rule in (("key16", KEY16), ("table", TABLE)):   # the rules by name, the other rule's input absent
        got_c, _ = _ops().her_select(b["pos"], b["terminated"], b["truncated"], b["age0"], name,
                                     key16=b["key16"] if rule == KEY16 else None,
                                     table=b["table"] if rule == TABLE else None, **KW)
        assert same_bits(host(got_c), hs.run_case(rule, fill=-1)[0])


@pytest.mark.parametrize("rule", RULES)
def test_one_step_and_no_step(rule):
    c = hs.cases()
    one = dict(pos=c["pos"][:1, :1], terminated=np.ones((1, 1), np.uint8), truncated=np.zeros((1, 1), np.uint8),
               age0=np.zeros(1, np.int32), key16=c["key16"][:1, :1], table=c["table"])
    for T in (1, 0):
        a = {k: (v[:T] if k in ("pos", "terminated", "truncated", "key16") else v) for k, v in one.items()}
        b = {k: _d(np.array(v)) for k, v in a.items()}
        ch = torch.full((T, 1, 4), SENTINEL, dtype=torch.int32, device=DEV)
        got_c, got_s = _ops().her_select(b["pos"], b["terminated"], b["truncated"], b["age0"], rule, key16=b["key16"],
                                         table=b["table"], choices=ch)
        want_c, want_s, _ = hs.select(a["pos"], a["terminated"], a["truncated"], a["age0"], rule, key16=a["key16"],
                                      table=a["table"], choices=np.full((T, 1, 4), SENTINEL, np.int32))
        assert same_bits(host(got_c), want_c) and same_bits(host(got_s), want_s)
        assert host(got_s).tolist() == [T, 0, 0, 0, 0, 0] and (host(got_c) == -1).all()


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("skip", [0, 4])
def test_relabel_on_the_kernels_choices_equals_the_oracle_on_the_restatements(on_device, rule, skip):
    c, b = hs.cases(), on_device
    reward = np.random.default_rng(5).random((CASE_T, CASE_N)).astype(np.float32)
    for max_goals in (1, 4):
        ch, st = _select(b, rule, max_goals, skip)
        got = _ops().her_relabel(b["pos"], b["terminated"], b["truncated"], b["age0"], _d(reward), ch, max_goals=max_goals,
                                 skip=skip)
        want = her_oracle.relabel(c["pos"], c["terminated"], c["truncated"], c["age0"], reward,
                                  choices=hs.reference(rule, max_goals, skip)[0], max_goals=max_goals, skip=skip)
        for k in KEYS:
            assert same_bits(host(got[k]), want[k]), (k, max_goals)
        assert int(host(st)[3]) == int(want["counts"].sum()) > 0 and int(host(st)[2]) == int(want["done"].sum())


def test_stats_accumulate_over_two_calls(on_device):
    _, st = _select(on_device, KEY16)
    once = host(st).copy()
    _, st2 = _select(on_device, KEY16, stats=st)
    assert st2 is st and same_bits(host(st), 2 * once) and same_bits(once, hs.reference(KEY16)[1])
    choices, none = torch.full((CASE_T, CASE_N, 4), SENTINEL, dtype=torch.int32, device=DEV), None
    b = on_device                                             # stats == NULL through the C ABI: the choices alone
    rc = _lib().ppo_her_select(_P(b["pos"]), _P(b["terminated"]), _P(b["truncated"]), _P(b["age0"]), CASE_T, CASE_N, 4, 0,
                               KEY16, _P(b["key16"]), None, 0, 0, 11, 3, 100, _P(choices), none, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and same_bits(host(choices), hs.reference(KEY16)[0])


def test_env_id0_and_step0_shift_the_tie_break(on_device):
    base = hs.reference(KEY16)[0]
    for kw in (dict(env_id0=4), dict(step0=101), dict(seed=11 + (1 << 32)), dict(env_id0=0xFFFFFFFE, step0=0xFFFFFFF0)):
        want = hs.run_case(KEY16, **{**KW, **kw})[0]
        assert not np.array_equal(want, base), kw
        assert same_bits(host(_select(on_device, KEY16, **kw)[0]), want), kw
    # env_id0 + n and step0 + t1 are all that enters: the same episodes one env further along see the shifted words
    want = hs.run_case(KEY16, env_id0=2, step0=101)[0]
    assert same_bits(host(_select(on_device, KEY16, env_id0=2, step0=101)[0]), want)


def test_rejections_write_nothing(on_device):
    b = on_device
    room = 16
    choices = torch.full((CASE_T * CASE_N * 4 + room,), SENTINEL, dtype=torch.int32, device=DEV)
    stats = torch.full((6 + room,), 5, dtype=torch.int64, device=DEV)
    canaries = [(choices, SENTINEL), (stats, 5)]
    good = dict(pos=_P(b["pos"]), terminated=_P(b["terminated"]), truncated=_P(b["truncated"]), age0=_P(b["age0"]), T=CASE_T,
                N=CASE_N, max_goals=4, skip=0, rule=TABLE, key16=_P(b["key16"]), table=_P(b["table"]), width=SIDE,
                height=SIDE, seed=11, env_id0=3, step0=100, choices=_P(choices), stats=_P(stats))
    bad = [{k: None} for k in ("pos", "terminated", "truncated", "age0", "choices")]
    bad += [dict(T=-1), dict(N=0), dict(N=-1), dict(max_goals=0), dict(max_goals=5), dict(max_goals=-1), dict(skip=-1),
            dict(skip=64), dict(rule=3), dict(rule=-1), dict(rule=KEY16, key16=None), dict(table=None), dict(width=0),
            dict(width=33), dict(height=0), dict(height=33), dict(T=1 << 20, N=1 << 20)]
    bad += [dict(pos=_P(b["pos"], 4)), dict(choices=_P(choices, 2)), dict(rule=KEY16, key16=_P(b["key16"], 1)),
            dict(table=_P(b["table"], 4)), dict(stats=_P(stats, 4))]
    for kw in bad:
        assert rejected("ppo_her_select", list({**good, **kw}.values()), canaries), kw
    # what the rules do not read may be anything: LATE without keys and with sides out of range, T = 0 with stats
    for kw in (dict(rule=LATE, key16=None, table=None, width=0, height=99), dict(rule=KEY16, table=None, width=-1),
               dict(rule=TABLE, key16=None)):
        rc = _lib().ppo_her_select(*{**good, **kw}.values(), _stream())
        torch.cuda.synchronize()
        assert rc == 0, kw
    assert not bool((choices == SENTINEL).all())
    choices.fill_(SENTINEL)
    stats.fill_(5)
    assert _lib().ppo_her_select(*{**good, "T": 0}.values(), _stream()) == 0
    torch.cuda.synchronize()
    assert all(bool((t == v).all()) for t, v in canaries)      # T == 0: accepted, nothing launched


# ------------------------------------------------------------------------------------------------ streams and capture
FILL = np.frombuffer(b"\xab" * 4, np.int32)[0]                 # stream_util.sentinel_ as an int32


def _stream_case(rule):
    def make(seed):
        c, r = hs.cases(), streams.rng(seed, 77 + rule)

        def roll(a):                                           # the same episodes on other envs: same shapes, other picks
            return np.roll(a, seed, axis=1)
        return streams.up(dict(pos=roll(c["pos"]), terminated=roll(c["terminated"]), truncated=roll(c["truncated"]),
                               age0=np.roll(c["age0"], seed), key16=r.integers(0, 5, (CASE_T, CASE_N)).astype(np.uint16),
                               table=r.integers(-9, 9, SIDE * SIDE + 1).astype(np.int64),
                               stats=r.integers(0, 100, 6).astype(np.int64)))

    def call(b, o, ctx):
        _ops().her_select(b["pos"], b["terminated"], b["truncated"], b["age0"], rule, key16=b["key16"], table=b["table"],
                          width=SIDE, height=SIDE, seed=9, env_id0=1, step0=7, choices=o["choices"], stats=b["stats"])
        return dict(choices=o["choices"], stats=b["stats"])

    def ref(h):
        ch, st, _ = hs.select(h["pos"], h["terminated"], h["truncated"], h["age0"], rule, key16=h["key16"], table=h["table"],
                              width=SIDE, height=SIDE, seed=9, env_id0=1, step0=7,
                              choices=np.full((CASE_T, CASE_N, 4), FILL, np.int32), stats=h["stats"])
        return dict(choices=ch, stats=st)

    return Case("her_select rule %d" % rule, "replay", ["ppo_her_select"], make, call, ref=ref, state=("stats",),
                outs=lambda: dict(choices=torch.empty((CASE_T, CASE_N, 4), dtype=torch.int32, device=DEV)))


STREAM_CASES = [_stream_case(rule) for rule in RULES]
# test_streams_gpu's completeness check reads its module's CASES when it runs and wants a case for every prototype that
# takes a stream, and that file is not this change's to edit.  A new list, not an append: the parametrised tests over
# there keep the list they were given, so these cases run once, here.  Run without this module imported, that check names
# ppo_her_select as uncovered; an entry in that file's own table is the maintainers' to make.
streams.CASES = streams.CASES + STREAM_CASES


@pytest.mark.parametrize("case", STREAM_CASES, ids=repr)
def test_eager_on_a_side_stream_behind_the_delay(case):
    streams.test_eager_on_a_side_stream(case)


@pytest.mark.parametrize("case", STREAM_CASES, ids=repr)
def test_captured_and_replayed_twice(case):
    streams.test_captured_and_replayed(case)


# ------------------------------------------------------------------------------------------------------------ trainer
TR_N, TR_T = 16, 64
TRAINER_RULES = {"late": LATE, "near": KEY16, "rare": TABLE}


@pytest.fixture(scope="module")
def trainer():
    """One v6 trainer (16 envs, T = 64, max_steps = 50, seeded) two rollouts in: the first one relabelled, counted and
    carried over, so that the history window of the second is not empty and the visit matrix is not zero."""
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    torch.manual_seed(2)
    eng = TwoarmyEngine(6, TR_N, 17, seed=9981, max_steps=50)
    agent = PPO()
    agent.K_epochs = 1
    tr = VecPPOTrainer(agent, eng, rollout_steps=TR_T, minibatch=1024, value_chunk=2048)
    gen = torch.Generator().manual_seed(41)
    tr.collect(uniforms=torch.rand(TR_T, TR_N, generator=gen).to(tr.device))
    tr.relabel()
    tr.account_visits(tr.her)
    tr.carry_over()
    tr.collect(uniforms=torch.rand(TR_T, TR_N, generator=gen).to(tr.device))
    assert len(tr._hist) == 1 and tr.her_select_rule is None
    yield tr
    eng.close()


def _window(tr):
    """The arrays relabel() concatenates, on the host, and the global step of their first row."""
    hist = list(tr._hist)

    def cat(i, cur):
        return np.concatenate([host(x[i]) for x in hist] + [host(cur)])
    back = TR_T * len(hist)
    return dict(pos=cat(0, tr.pos[4:4 + TR_T]), terminated=cat(1, tr.term), truncated=cat(2, tr.trunc),
                reward=cat(3, tr.reward_train), age0=host(hist[0][4]), back=back, step0=tr.env_steps // TR_N - TR_T - back)


def _cut(rec, back):
    keep = rec["t"] >= back
    out = {k: np.ascontiguousarray(rec[k][keep]) for k in ("t", "n", "goal", "reward", "done")}
    out["t"] = out["t"] - np.int32(back)
    out["counts"] = np.bincount(out["n"], minlength=TR_N).astype(np.int32)
    return out


@pytest.mark.parametrize("name", list(TRAINER_RULES))
def test_trainer_relabel_equals_the_restatement_over_the_window(trainer, name):
    from twoarmy_amd import minigrid_nav as nav
    tr, w = trainer, _window(trainer)
    tr.enable_her_select(name)
    key16 = table = None
    if name == "near":                                        # the rule's inputs, as the device holds them before the call
        key16 = host(nav.as_int(nav.lookup(tr._static_field(reuse=True), _d(w["pos"]), 17, 17))).astype(np.uint16)
        assert (key16 != 0xFFFF).any()
    if name == "rare":
        table = host(tr.visits.cumulative).copy()
        assert table.sum() >= TR_T * TR_N and table.max() > 1            # the first rollout and its records, counted
    got = {k: host(v) for k, v in tr.relabel().items()}
    choices, stats, _ = hs.select(w["pos"], w["terminated"], w["truncated"], w["age0"], TRAINER_RULES[name], key16=key16,
                                  table=table, seed=tr.her_seed, env_id0=tr.engine.env_id0, step0=w["step0"])
    whole = her_oracle.relabel(w["pos"], w["terminated"], w["truncated"], w["age0"], w["reward"], choices=choices)
    want = _cut(whole, w["back"])
    assert (whole["t"] < w["back"]).any() and want["t"].size > 0          # the window matters, and so does the cut
    for k in KEYS:
        assert same_bits(got[k], want[k]), (name, k)
    s = tr.her_select_stats()
    assert s["picks"] == int(stats[2]) > 0 and s["episodes"] == int(stats[0]) and s["unreachable"] == int(stats[5])
    assert s["mean_prefix"] == int(stats[3]) / int(stats[2]) == whole["t"].size / int(stats[2])
    assert (s["mean_key"] is None) == (name == "late")
    # downstream: the records keep the run pattern, one-step targets and GAE along the runs
    ag = tr.agent
    try:
        ag.gae_lambda, ag.use_done_mask, tr.her_gae = 0.0, False, False
        adv, ct = tr.compute_targets()
        assert tr.her_out_of_pattern == 0 and adv.numel() == TR_T * TR_N + want["t"].size
        ag.gae_lambda, ag.use_done_mask, tr.her_gae = 0.95, True, True
        adv, ct = tr.compute_targets()
        assert tr.her_out_of_pattern == 0 and bool(torch.isfinite(adv).all()) and bool(torch.isfinite(ct).all())
        assert same_bits(host(tr.her_targets["run_end"]), (want["done"] != 0).astype(np.uint8))   # cut at the runs' ends
    finally:
        ag.gae_lambda, ag.use_done_mask, tr.her_gae = 0.0, False, False
        tr.enable_her_select(None)


def test_trainer_without_a_rule_relabels_as_before(trainer):
    """relabel() with no rule, before and after a rule was on, == the call the trainer made before it knew of rules: the
    reference's draw over the window, cut at `back`; explicit choices are not overridden by a rule."""
    tr, w = trainer, _window(trainer)
    assert tr.her_select_rule is None and tr.her_select_stats() is None
    before = {k: host(v) for k, v in tr.relabel().items()}
    tr.enable_her_select("late")
    late = {k: host(v) for k, v in tr.relabel().items()}
    explicit = torch.full((TR_T, TR_N, 4), -1, dtype=torch.int32, device=DEV)
    assert tr.relabel(choices=explicit)["t"].numel() == 0
    tr.enable_her_select(None)
    after = {k: host(v) for k, v in tr.relabel().items()}
    h = _ops().her_relabel(_d(w["pos"]), _d(w["terminated"]), _d(w["truncated"]), _d(w["age0"]), _d(w["reward"]), None,
                           seed=tr.her_seed, env_id0=tr.engine.env_id0, step0=w["step0"], max_goals=4, skip=0)
    plain = _cut({k: host(v) for k, v in h.items()}, w["back"])
    for k in KEYS:
        assert same_bits(before[k], after[k]) and same_bits(before[k], plain[k]), k
    assert not (late["t"].size == before["t"].size and np.array_equal(late["goal"], before["goal"]))
    with pytest.raises(ValueError):
        tr.enable_her_select("best")
