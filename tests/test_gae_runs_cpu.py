"""GAE along hindsight runs without a GPU: the float64 reference (gae_runs_ref.py) against the oracle's column scan and
the one-step formula, the numpy restatement of ppo_run_ends on hand-made records, the ctypes mirror of the three new
entry points, and the entry point's flag and relabelling rule."""
import itertools
import os
import re

import numpy as np

import gae_runs_ref as gr
import ppo_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ppo_run_ends": 8, "ppo_gae_runs": 14, "ppo_gae_runs_workspace": 1}


def _dyadic_tile(T, N, seed):
    """Multiples of 1/16 of magnitude < 4 and done flags: with gamma = lambda = 1/2 every product and sum of a T <= 6
    scan is exact in float32 (c^5 = 2^-10 on a 2^-5 grid, magnitudes < 2^5: 20 bits), so float32 and float64 agree."""
    rs = np.random.RandomState(seed)
    r, v, nv = (rs.randint(-63, 64, (T, N)).astype(np.float32) / 16 for _ in range(3))
    done = (rs.rand(T, N) < 0.3).astype(np.uint8)
    done[T - 1] = 1                                                # one run per column at least: the column's end
    return r, v, nv, done


def test_reference_equals_the_oracle_column_by_column():
    T, N = 6, 37
    r, v, nv, done = _dyadic_tile(T, N, 5)
    want_adv, want_tgt, want_ret = po.gae(r, v, nv, done, 0.5, 0.5, True)
    flat = lambda x: np.ascontiguousarray(x.T).reshape(-1)         # noqa: E731  env-major: a column is a stretch of records
    adv, tgt, ret, S, L = gr.gae_runs64(flat(r), flat(v), flat(nv), flat(done), flat(done), 0.5, 0.5, True)
    for got, want in ((adv, want_adv), (tgt, want_tgt), (ret, want_ret)):
        assert np.array_equal(got.reshape(N, T).T, want.astype(np.float64))
    assert (L >= 1).all() and L.reshape(N, T)[:, T - 1].tolist() == [1] * N and (S >= 0).all()
    # runs end at the done flags: L counts down to each of them
    d = flat(done)
    assert all(L[j] == 1 for j in np.nonzero(d)[0]) and all(L[j] == L[j + 1] + 1 for j in np.nonzero(d == 0)[0])


def test_reference_with_every_run_end_set_is_the_one_step_formula():
    H = 300
    r, v, nv = gr.inputs(H, 3)
    done = gr.dones(gr.pattern("her", H), 3)
    for (gamma, lam), mask in itertools.product([(0.99, 0.0), (0.99, 0.95), (1.0, 1.0)], (False, True)):
        for run_end in (np.ones(H, np.uint8), gr.pattern("her", H)):
            if lam != 0.0 and not run_end.all():
                continue
            adv, tgt, ret, S, L = gr.gae_runs64(r, v, nv, done, run_end, gamma, lam, mask)
            cut = 1.0 - done if mask else np.ones(H)
            t64 = r.astype(np.float64) + float(np.float32(gamma)) * nv.astype(np.float64) * cut
            assert np.array_equal(tgt, t64) and np.array_equal(adv, t64 - v) and np.array_equal(ret, adv + v)
            assert (L == 1).all() and np.array_equal(S, np.abs(r.astype(np.float64)) + np.abs(
                float(np.float32(gamma)) * nv.astype(np.float64)) + np.abs(v.astype(np.float64)))
            t32, d32 = gr.one_step32(r, v, nv, done, gamma, mask)
            assert np.abs(t32 - tgt).max() <= 2 * gr.EPS32 * S.max() and np.abs(d32 - adv).max() <= 2 * gr.EPS32 * S.max()


def test_reference_keeps_the_bootstrap_at_a_done_record_without_the_mask():
    """One run of three records ending done: without the mask the last record keeps gamma * nv (PPO.py:113), with it the
    bootstrap goes; the run end cuts the scan in both, so the record behind (a run of its own) never enters."""
    r = np.array([0.0, 0.0, 0.75, 5.0], np.float32)
    v = np.zeros(4, np.float32)
    nv = np.array([1.0, 1.0, 2.0, 7.0], np.float32)
    done = np.array([0, 0, 1, 1], np.uint8)
    end = np.array([0, 0, 1, 1], np.uint8)
    adv, tgt, _, _, L = gr.gae_runs64(r, v, nv, done, end, 0.5, 0.5, False)
    assert tgt.tolist() == [0.5, 0.5, 1.75, 8.5] and adv.tolist() == [0.5 + 0.25 * (0.5 + 0.25 * 1.75), 0.5 + 0.25 * 1.75, 1.75, 8.5]
    assert L.tolist() == [3, 2, 1, 1]
    adv, tgt, _, _, _ = gr.gae_runs64(r, v, nv, done, end, 0.5, 0.5, True)
    assert tgt.tolist() == [0.5, 0.5, 0.75, 5.0] and adv.tolist() == [0.5 + 0.25 * (0.5 + 0.25 * 0.75), 0.5 + 0.25 * 0.75, 0.75, 5.0]


def test_run_ends_restatement_on_hand_made_records():
    t = np.array([3, 4, 5, 0, 1, 2, 3, 9, 10, 4], np.int32)
    n = np.array([1, 1, 1, 1, 1, 2, 2, 2, 2, 2], np.int32)
    goal = np.array([[1, 2]] * 3 + [[3, 4]] * 2 + [[3, 4]] * 2 + [[0.0, 5]] + [[-0.0, 5]] + [[np.nan, 1]], np.float32)
    done = np.array([0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.uint8)
    end, broken = gr.run_ends(t, n, goal, done)
    #   0-2: a run ending done; 3-4: a run broken by the env change at 5; 5-6: ends done; 7-8: -0.0 links with +0.0;
    #   8 -> 9: t is not +1 (and the goal is NaN); 9: the last record never links
    assert end.tolist() == [0, 0, 1, 0, 1, 0, 1, 0, 1, 1] and broken == 3
    for k in (0, 1):                                               # either goal component alone breaks the run
        g2 = goal.copy()
        g2[1, k] += 1
        assert gr.run_ends(t, n, g2, done)[0][:3].tolist() == [1, 1, 1]
    g2 = goal.copy()
    g2[0:2] = np.nan                                               # NaN == NaN is false: no link
    assert gr.run_ends(t, n, g2, done)[0][:2].tolist() == [1, 1]
    d2 = done.copy()
    d2[0] = 1                                                      # done in mid-run: a run end, not a broken record
    e2, b2 = gr.run_ends(t, n, goal, d2)
    assert e2.tolist() == [1] + end.tolist()[1:] and b2 == 3
    one = gr.run_ends(t[:1], n[:1], goal[:1], done[:1])
    assert one[0].tolist() == [1] and one[1] == 1


def test_patterns_are_what_they_say():
    assert gr.pattern("singletons", 65).all()
    e = gr.pattern("runs64", 257)
    assert np.nonzero(e)[0].tolist() == [63, 127, 191, 255, 256]
    e = gr.pattern("runs64+1", 257)
    assert np.nonzero(e)[0].tolist() == [0, 64, 128, 192, 256]
    e = gr.pattern("her", 70001)
    lengths = np.diff(np.concatenate([[-1], np.nonzero(e)[0]]))
    assert lengths.min() >= 1 and lengths.max() <= 64 and lengths.sum() == 70001
    e = gr.pattern("one1000", 70001)
    lengths = np.diff(np.concatenate([[-1], np.nonzero(e)[0]]))
    assert lengths.max() == 1000 and e[2048 - 300 + 999] == 1 and not e[2048 - 300:2048 - 300 + 999].any()
    assert np.nonzero(gr.pattern("whole", 1000))[0].tolist() == [999]


def test_edge_table_and_boundary_runs_are_what_they_say():
    assert gr.EDGES == (64, 512, 2048, 131072, 1048576, 4194304) and gr.EDGE_NAMES[131072] == "chunk1"
    assert gr.boundaries(64) == [] and gr.boundaries(65) == [64] and gr.boundaries(2048 * 2048) == list(gr.EDGES[:5])
    assert gr.boundaries(2048 * 2048 + 1) == list(gr.EDGES)
    lengths = np.diff(np.concatenate([[-1], np.nonzero(gr.pattern("her16", 70001))[0]]))
    assert lengths.min() >= 1 and lengths.max() == 16 and lengths.sum() == 70001
    H = 64 * 2048 + 1
    B = gr.boundaries(H)
    e, placed = gr.boundary_runs(H, B, "ends", True)
    assert placed == [(b - 4 + 4 * k, min(b - 1 + 4 * k, H - 1)) for b in B for k in (0, 1)]
    assert all(e[a - 1] and e[b] and not e[a:b].any() for a, b in placed)
    e, placed = gr.boundary_runs(H, B, "straddle", True)
    assert placed == [(b - 3, min(b + 2, H - 1)) for b in B] and all(e[a - 1] and e[b] and not e[a:b].any() for a, b in placed)
    d = gr.boundary_dones(e, B, "straddle", 0)
    assert all(d[b - 1] and not e[b - 1] for b in B) and (d[e != 0] == 1).all()
    e, placed = gr.boundary_runs(H, B, "long", False)
    assert placed == [(40, 87), (384, 639), (1024, 3071), (H - 1 - 2 * 2048, H - 1)]
    assert all(e[a - 1] and e[b] and not e[a:b].any() for a, b in placed)
    d = gr.boundary_dones(e, B, "long", 0)
    assert all(d[b] for b in B) and not e[[64, 512, 2048]].any()


def _exact_cases(H):
    """(family, run_end, done) over the background patterns and every placement of the boundary sweep that fits H."""
    for family in gr.FAMILIES:
        short = family != "c1"
        for kind in ("singletons", "her16", "whole") if short and H <= 16 else ("singletons", "her16") if short else (
                "singletons", "runs64", "runs64+1", "her", "whole"):
            end = gr.pattern(kind, H, H)
            yield family, kind, end, gr.dones(end, H)
        for variant in gr.variants(family):
            end, _ = gr.boundary_runs(H, gr.boundaries(H), variant, short, H)
            yield family, variant, end, gr.boundary_dones(end, gr.boundaries(H), variant, H)


def test_exact_reference_equals_the_float64_loop():
    for H in (1, 65, 2049, 5000):
        for family, name, end, done in _exact_cases(H):
            gamma, lam = gr.FAMILIES[family]
            r, v, nv = gr.exact_inputs(family, H, H)
            for mask in (False, True):
                want = gr.gae_runs64(r, v, nv, done, end, gamma, lam, mask)[:3]
                got = gr.exact_runs(r, v, nv, done, end, gamma, lam, mask)
                for g, w in zip(got, want):
                    assert g.dtype == np.float64 and np.array_equal(g, w), (H, family, name, mask)
                t32, d32 = gr.one_step32(r, v, nv, done, gamma, mask)      # the one-step formula in float32 is exact too
                assert np.array_equal(t32.astype(np.float64), want[1])
                assert np.array_equal((got[0].astype(np.float32) + v).astype(np.float64), want[2])


def test_exact_inputs_use_all_three_arrays_and_the_mask_changes_delta():
    H = 5000
    for family, (gamma, lam) in gr.FAMILIES.items():
        r, v, nv = gr.exact_inputs(family, H, 1)
        assert all(len(np.unique(x)) > 5 for x in (r, v, nv))
        end, _ = gr.boundary_runs(H, gr.boundaries(H), "straddle", family != "c1", 1)
        done = gr.boundary_dones(end, gr.boundaries(H), "straddle", 1)
        off, on = (gr.exact_runs(r, v, nv, done, end, gamma, lam, m) for m in (False, True))
        assert not np.array_equal(off[0], on[0]) and not np.array_equal(off[1], on[1])
        lone = gr.exact_runs(r, v, nv, done, np.ones(H, np.uint8), gamma, lam, False)
        assert not np.array_equal(off[0], lone[0])                     # and the runs enter the advantage


def test_exactness_assertion_fires_on_inputs_that_are_too_large():
    import pytest
    one = np.zeros(4, np.uint8)
    z = np.zeros(4, np.float32)
    big = np.full(4, 2.0 ** 23, np.float32)                            # suffix sums up to 2^25
    with pytest.raises(AssertionError, match="does not fit float32"):
        gr.exact_runs(big, z, z, one, one, 1.0, 1.0, False)
    assert gr.exact_runs(big / 4, z, z, one, one, 1.0, 1.0, False)[0].tolist() == [2.0 ** 23, 3 * 2.0 ** 21, 2.0 ** 22, 2.0 ** 21]
    gr.exact_runs(big, z, z, one, np.ones(4, np.uint8), 1.0, 1.0, False)       # cut into singletons they fit
    up_down = np.array([2.0 ** 23, 2.0 ** 23, -2.0 ** 23, -2.0 ** 23], np.float32)
    with pytest.raises(AssertionError, match="does not fit float32"):    # a piece in mid-run, not only the suffix sums
        gr.exact_runs(up_down, z, z, one, one, 1.0, 1.0, False)
    for gamma, lam in ((0.5, 1.0), (1.0, 0.5)):
        e30 = np.zeros(30, np.uint8)
        d30 = np.full(30, 15, np.float32)
        with pytest.raises(AssertionError, match="need 34 bits"):        # a run of 30: 29 + 5 bits
            gr.exact_runs(d30, 0 * d30, 0 * d30, e30, e30, gamma, lam, False)
        e30[15::16] = 1
        gr.exact_runs(d30, 0 * d30, 0 * d30, e30, e30, gamma, lam, False)      # runs of 16: 20 bits
        with pytest.raises(AssertionError, match="need 28 bits"):        # magnitudes < 2^13 in runs of 16
            gr.exact_runs(d30 * 256, 0 * d30, 0 * d30, e30, e30, gamma, lam, False)
        with pytest.raises(AssertionError):                            # a delta that is no integer
            gr.exact_runs(d30 / 2, 0 * d30, 0 * d30, e30, e30, gamma, lam, False)


def test_ctypes_table_and_header_agree_on_the_new_entry_points():
    from twoarmy_amd import _lib
    txt = open(os.path.join(ROOT, "include", "twoarmy_ppo.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, arity in NEW.items():
        m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name, txt)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == arity == len(_lib._SIGS[name][1]), name
        assert name in _lib.exported_symbols()
        if arity > 1:
            assert params[-1] == "void *stream", name             # the spelling tests/test_streams_gpu.py lists entries by


def test_parser_accepts_her_gae_and_it_is_off_by_default():
    from twoarmy_amd.soa.train_ppo import build_parser
    p = build_parser()
    assert p.parse_args([]).her_gae is False
    a = p.parse_args(["--her_gae", "--gae_lambda", "0.95"])
    assert a.her_gae is True and a.gae_lambda == 0.95


def test_relabel_wanted_truth_table():
    from twoarmy_amd.soa.train_ppo import relabel_wanted
    table = {(True, 0.0, False): True, (True, 0.0, True): True, (True, 0.95, False): False, (True, 0.95, True): True,
             (False, 0.0, False): False, (False, 0.0, True): False, (False, 0.95, False): False, (False, 0.95, True): False}
    for (her, lam, her_gae), want in table.items():
        assert relabel_wanted(her, lam, her_gae) is want, (her, lam, her_gae)


def test_her_gae_is_refused_for_the_window_record_agents():
    import pytest
    from twoarmy_amd.soa import train_ppo
    for kw in (dict(predictor=True), dict(soa=True)):
        with pytest.raises(SystemExit, match="--her_gae"):
            train_ppo.main(["--her_gae", "--gae_lambda", "0.95"], **kw)
