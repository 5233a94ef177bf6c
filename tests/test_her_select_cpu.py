"""tests/her_select_ref.py, the numpy restatement of ppo_her_select, against things it does not define itself: what
oracle/her_oracle.relabel makes of its choices, what each rule means, which rows it leaves alone, and what its Philox
tie-break depends on.  Also the host side of the feature: the ctypes row, the flag, the log field."""
import numpy as np
import pytest

import her_oracle
import her_select_ref as hs
from her_select_ref import KEY16, LATE, SENTINEL, TABLE, UNREACHABLE

RULES = (LATE, KEY16, TABLE)


def _relabel(choices, max_goals, skip):
    c = hs.cases()
    reward = np.zeros(c["terminated"].shape, np.float32)
    return her_oracle.relabel(c["pos"], c["terminated"], c["truncated"], c["age0"], reward, choices=choices,
                              max_goals=max_goals, skip=skip)


def _runs(rec):
    """(n, first t, last t) of every run of the oracle's records: a run ends with its done record."""
    ends = np.flatnonzero(rec["done"])
    starts = np.concatenate([[0], ends[:-1] + 1])
    return [(int(rec["n"][e]), int(rec["t"][s]), int(rec["t"][e])) for s, e in zip(starts, ends)]


def test_the_shared_cases_hold_every_edge():
    hs.check_cases_present()


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("skip", [0, 4])
def test_relabel_emits_what_stats_promise(rule, skip):
    """stats[3] = the records her_oracle.relabel emits from these choices, stats[2] = its runs: every pick is used."""
    for max_goals in (1, 2, 3, 4):
        choices, stats, eps = hs.reference(rule, max_goals, skip)
        rec = _relabel(choices, max_goals, skip)
        assert int(rec["counts"].sum()) == int(stats[3]) == rec["t"].size
        assert int(rec["done"].sum()) == int(stats[2])
        assert int(stats[0]) == sum(e["handled"] for e in eps) and int(stats[1]) == sum(len(e["idx"]) for e in eps if e["handled"])
    assert stats[3] > 0


def test_late_with_one_goal_is_one_run_up_to_the_last_first_visit():
    choices, _, eps = hs.reference(LATE, 1, 0)
    c = hs.cases()
    want = []
    for e in eps:
        if e["handled"]:
            fv = her_oracle.first_visit(c["pos"][e["s0"]:e["t1"] + 1, e["n"]])
            if fv.max() > 0:                                             # C >= 1
                want.append((e["n"], e["s0"], e["s0"] + int(fv.max())))
    assert len(want) > 5 and _runs(_relabel(choices, 1, 0)) == want


@pytest.mark.parametrize("rule", [KEY16, TABLE])
def test_every_pick_has_a_key_no_larger_than_every_candidate_left(rule):
    for max_goals in (1, 3, 4):
        for e in hs.reference(rule, max_goals, 0)[2]:
            if e["handled"] and e["picks"]:
                left = [e["key"][c] for c in range(len(e["key"])) if c not in e["picks"]]
                assert not left or max(e["key"][c] for c in e["picks"]) <= min(left)
                assert [e["key"][c] for c in e["picks"]] == sorted(e["key"][c] for c in e["picks"])   # and in key order


def test_near_takes_the_nearest_cells_of_the_key_array():
    """KEY16 against the array itself: the picked records' keys are the k smallest among the episode's first visits
    behind the first, read from key16 by (t, n)."""
    c = hs.cases()
    choices, _, eps = hs.reference(KEY16, 4, 0)
    for e in eps:
        if not e["handled"]:
            continue
        fv = her_oracle.first_visit(c["pos"][e["s0"]:e["t1"] + 1, e["n"]])
        keys = sorted(int(c["key16"][e["s0"] + i, e["n"]]) for i in fv if i > 0)
        row = choices[e["t1"], e["n"]]
        got = sorted(int(c["key16"][e["s0"] + fv[r], e["n"]]) for r in row if r >= 0)
        assert got == keys[:4]


@pytest.mark.parametrize("rule", RULES)
def test_rows_fill_and_distinct_picks(rule):
    for max_goals in (1, 2, 3, 4):
        for skip in (0, 4):
            choices, _, eps = hs.reference(rule, max_goals, skip)
            written = np.zeros(choices.shape[:2], bool)
            for e in eps:
                if not e["handled"]:
                    continue
                row = choices[e["t1"], e["n"]]
                k = min(max_goals, len(e["idx"]))
                written[e["t1"], e["n"]] = True
                assert (row[k:] == -1).all() and (row[:k] >= 0).all() and (row[:k] < e["U"]).all()
                assert len(set(row[:k].tolist())) == k                   # distinct ranks
                assert set(row[:k].tolist()) <= set(e["rank"])           # and never the first visit at record `skip`
            assert (choices[~written] == SENTINEL).all() and (choices[written] != SENTINEL).all()
            assert 0 < written.sum() < written.size


def test_the_tie_break_follows_the_seed_and_nothing_else():
    """All keys of the episode (2, 14, 33) are equal under KEY16, so its order is Philox's: it moves with the seed (either
    word), with env_id0 and step0 only as env_id0 + n and step0 + t1, and not with max_goals or the other rules' inputs."""
    def order(**kw):
        eps = hs.run_case(KEY16, **kw)[2]
        e = [e for e in eps if e["handled"] and (e["n"], e["s0"], e["t1"]) == (2, 14, 33)][0]
        return [e["rank"][c] for c in sorted(range(len(e["rank"])), key=lambda c: (e["key"][c], e["word"][c]))]
    base = order()
    assert len(base) > 4 and base != sorted(base)
    assert order(seed=12) != base and order(seed=11 + (1 << 32)) != base
    assert order(max_goals=1) == base
    assert order(env_id0=4) != base and order(step0=101) != base
    e = hs.reference(KEY16)[2]
    words = {(x["n"], x["t1"]): x["word"] for x in e if x["handled"]}
    shifted = {(x["n"], x["t1"]): x["word"] for x in hs.run_case(KEY16, env_id0=2, step0=101)[2] if x["handled"]}
    assert shifted[3, 29] != words[3, 29]
    c = hs.cases()                                                       # the word is a function of (seed, env, step, rank)
    assert words[2, 33] == [hs.tie_word(11, 3 + 2, 100 + 33, r) for r in
                            [x for x in e if x["handled"] and (x["n"], x["t1"]) == (2, 33)][0]["rank"]]
    assert c["key16"][14:34, 2].tolist() == [7] * 20


def test_stats_accumulate_and_leave_unreachable_keys_out():
    _, once, eps = hs.reference(KEY16)
    _, twice, _ = hs.run_case(KEY16, stats=once)
    assert (twice == 2 * once).all()
    picked = [e["key"][c] for e in eps if e["handled"] for c in e["picks"]]
    assert int(once[5]) == picked.count(UNREACHABLE) > 0
    assert int(once[4]) == sum(k for k in picked if k != UNREACHABLE)
    assert hs.reference(LATE)[1][4] == 0 and hs.reference(LATE)[1][5] == 0 and hs.reference(TABLE)[1][5] == 0
    assert int(hs.reference(TABLE)[1][4]) < -(1 << 39)                   # the 64-bit entry was picked and summed


def test_ctypes_row_flag_and_log_field():
    import ctypes as C
    import twoarmy_amd
    from twoarmy_amd import ppo_ops
    from twoarmy_amd.soa import train_ppo
    res, args = twoarmy_amd._lib._SIGS["ppo_her_select"]
    assert res is C.c_int and len(args) == 19 and args[13] is C.c_uint64 and args[14] is args[15] is C.c_uint32
    assert ppo_ops.HER_RULES == {"late": LATE, "key16": KEY16, "table": TABLE}
    p = train_ppo.build_parser()
    assert p.parse_args([]).her_select == "random"
    assert [p.parse_args(["--her_select", r]).her_select for r in ("late", "near", "rare")] == ["late", "near", "rare"]
    with pytest.raises(SystemExit):
        p.parse_args(["--her_select", "best"])
    line = train_ppo.select_fields("near", dict(picks=12, mean_prefix=7.25, mean_key=3.5, unreachable=2))
    assert line == " her_sel near picks 12 prefix 7.25 key 3.50 unreachable 2"
    assert train_ppo.select_fields("late", dict(picks=3, mean_prefix=9.0, mean_key=None, unreachable=0)).endswith("key - unreachable 0")
    assert train_ppo.select_fields("rare", None) == " her_sel rare -"
