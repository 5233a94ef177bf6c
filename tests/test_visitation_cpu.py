"""Visit counting, CPU side: the numpy restatement (tests/visit_ref.py) is the reference's quantity on the reference's
own recorded data, and the library, the ctypes table and the train_ppo parser know the new names.  The argument checks of
the two entry points run before any launch, so they need no device."""
import ctypes as C
import os
import re

import numpy as np

import visit_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_hist_is_the_reference_heatmap_loop_on_its_recorded_buffers():
    """heatmap.py:58-63 over buffer['p'][:, 4] of the 7 recorded her_func cases, before and after the hindsight copies."""
    bufs = VR.her_buffers()
    assert len(bufs) == 14
    for name, p in bufs:
        assert p.min() >= 0 and p.max() <= 15, name
        ref = VR.reference_heatmap(p)
        got = VR.visit_hist(p.reshape(-1, 1, 2), 17, 17)
        assert got[289] == 0 and got.sum() == len(p), name
        assert np.array_equal(got[:289].reshape(17, 17), ref.astype(np.int64)), name
    # the ring buffer keeps its size: the copies her_func wrote are what makes an "after" buffer differ from its "before"
    assert any(not np.array_equal(bufs[2 * c + 1][1], bufs[2 * c][1]) for c in range(7))


def test_restated_scan_is_np_unique_per_episode_on_recorded_traces():
    """env_buffer.py:138 `np.unique(p, axis=0, return_index=True)` per finished episode of the 16 random traces."""
    cols = VR.golden_columns()
    assert len(cols[6]) == 6 and len(cols[4]) == 10
    episodes = 0
    for variant, columns in cols.items():
        for pos, term, trunc in columns:
            first, cells, left = VR.visit_scan(pos.reshape(-1, 1, 2), term.reshape(-1, 1), trunc.reshape(-1, 1), 17, 17)
            done = np.nonzero(term | trunc)[0]
            start = 0
            for t in done.tolist():
                index, n_unique = VR.reference_goal_candidates(pos[start:t + 1])
                assert np.nonzero(first[start:t + 1, 0])[0].tolist() == index, (variant, start, t)
                assert cells[t, 0] == n_unique
                start = t + 1
                episodes += 1
            index, n_unique = VR.reference_goal_candidates(pos[start:]) if start < len(pos) else ([], 0)
            assert np.nonzero(first[start:, 0])[0].tolist() == index and len(left[0]) == n_unique   # the running episode
    assert episodes == 58


def test_restatement_does_not_depend_on_the_cut_and_the_carry_layout_round_trips():
    rng = np.random.default_rng(5)
    T, N, W, H = 70, 5, 9, 5
    pos = rng.integers(-1, 10, size=(T, N, 2)).astype(np.float32)
    term = (rng.random((T, N)) < 0.05).astype(np.uint8)
    trunc = (rng.random((T, N)) < 0.03).astype(np.uint8)
    seen0 = [set(rng.integers(0, W * H, 4).tolist()) for _ in range(N)]
    whole = VR.visit_scan(pos, term, trunc, W, H, seen0)
    seen, firsts, cells, t = seen0, [], [], 0
    for step in (1, 7, 40, 22):
        a, b, seen = VR.visit_scan(pos[t:t + step], term[t:t + step], trunc[t:t + step], W, H, seen)
        firsts.append(a); cells.append(b); t += step
    assert t == T and seen == whole[2]
    assert np.array_equal(np.concatenate(firsts), whole[0]) and np.array_equal(np.concatenate(cells), whole[1])
    assert VR.carry_to_sets(VR.sets_to_carry(seen, W, H), N, W, H) == seen
    assert VR.sets_to_carry([set()] * N, W, H).tolist() == [0] * (2 * N)
    # dense with the first-visit mask + the rest = everything; indexed over all records = dense
    full = VR.visit_hist(pos, W, H)
    assert np.array_equal(VR.visit_hist(pos, W, H, mask=whole[0]) + VR.visit_hist(pos, W, H, mask=1 - whole[0]), full)
    tt, nn = np.divmod(np.arange(T * N), N)
    assert np.array_equal(VR.visit_hist(pos, W, H, t_idx=tt, n_idx=nn), full) and full[W * H] > 0


def test_cell_rule_at_the_edges():
    W, H = 9, 5
    for bad in (np.nan, np.inf, -np.inf, -1.0, 1e9):
        assert VR.cell_of(bad, 0.0, W, H) == W * H and VR.cell_of(0.0, bad, W, H) == W * H
    assert VR.cell_of(float(H), 0.0, W, H) == W * H and VR.cell_of(0.0, float(W), W, H) == W * H
    assert VR.cell_of(H - 1.0, W - 1.0, W, H) == W * H - 1 and VR.cell_of(4.99, 8.5, W, H) == W * H - 1
    assert VR.cell_of(-0.0, -0.0, W, H) == 0                  # 0 <= -0.0 as a float comparison, and int(-0.0) = 0


def _host(n_bytes):
    return C.create_string_buffer(n_bytes)


def test_library_exports_the_symbols_and_rejects_bad_arguments_before_any_launch():
    txt = open(os.path.join(ROOT, "include", "twoarmy_ppo.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    import twoarmy_amd
    for name in ("ppo_visit_scan", "ppo_visit_carry_words", "ppo_visit_hist"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in twoarmy_amd._lib.exported_symbols(), name
    assert "PPO.py:161" in txt and "heatmap.py:58-81" in txt             # the reference lines the kernels replace
    n_args = {k: len(twoarmy_amd._lib._SIGS[k][1]) for k in ("ppo_visit_scan", "ppo_visit_carry_words", "ppo_visit_hist")}
    assert n_args == {"ppo_visit_scan": 11, "ppo_visit_carry_words": 3, "ppo_visit_hist": 11}
    lib = twoarmy_amd._lib.lib()
    assert lib.ppo_visit_carry_words(17, 17, 4096) == 10 * 4096 and lib.ppo_visit_carry_words(32, 32, 3) == 96
    assert lib.ppo_visit_carry_words(1, 1, 5) == 5 and lib.ppo_visit_carry_words(17, 17, 0) == 0
    for w, h, n in ((0, 17, 4), (17, 0, 4), (33, 17, 4), (17, 33, 4), (-1, 17, 4), (17, 17, -1)):
        assert lib.ppo_visit_carry_words(w, h, n) < 0, (w, h, n)

    buf = _host(4096)                                   # host memory: a rejected call never reads it
    p = C.addressof(buf)
    ok_scan = dict(pos=p, term=p, trunc=p, T=4, N=4, w=17, h=17, carry=p, fv=p, ec=p)
    ok_hist = dict(pos=p, T=4, N=4, mask=None, t=None, n=None, B=0, w=17, h=17, counts=p)

    def scan(**kw):
        a = dict(ok_scan, **kw)
        return lib.ppo_visit_scan(a["pos"], a["term"], a["trunc"], a["T"], a["N"], a["w"], a["h"], a["carry"], a["fv"],
                                  a["ec"], None)

    def hist(**kw):
        a = dict(ok_hist, **kw)
        return lib.ppo_visit_hist(a["pos"], a["T"], a["N"], a["mask"], a["t"], a["n"], a["B"], a["w"], a["h"], a["counts"],
                                  None)

    for bad in (dict(pos=None), dict(carry=None), dict(term=None), dict(trunc=None), dict(w=0), dict(w=33), dict(h=0),
                dict(h=33), dict(w=-3), dict(T=-1), dict(N=-1)):
        assert scan(**bad) < 0, bad
    for bad in (dict(pos=None), dict(counts=None), dict(w=0), dict(w=33), dict(h=0), dict(h=33), dict(T=-1), dict(N=-1),
                dict(B=-1), dict(t=p, B=2), dict(n=p, B=2)):
        assert hist(**bad) < 0, bad
    # nothing to do: 0, and nothing launched (these pointers are host memory)
    assert scan(T=0) == 0 and scan(N=0) == 0 and scan(T=0, fv=None, ec=None) == 0
    assert hist(T=0) == 0 and hist(N=0) == 0 and hist(t=p, n=p, B=0) == 0 and hist(T=0, t=p, n=p, B=3) == 0
    assert buf.raw == bytes(4096)


def test_parser_and_front_ends_know_the_new_names():
    from twoarmy_amd.soa import train_ppo
    p = train_ppo.build_parser()
    assert p.parse_args([]).visit_dir is None and p.parse_args([]).track_buffer_file is None
    assert p.parse_args(["--visit_dir", "x"]).visit_dir == "x"
    from twoarmy_amd import ppo_ops, visitation
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    assert callable(ppo_ops.visit_scan) and callable(ppo_ops.visit_hist) and visitation.VisitTracker
    assert callable(VecPPOTrainer.account_visits) and callable(VecPPOTrainer.visit_stats)


def test_log_tail_of_visit_dir():
    from twoarmy_amd.soa.train_ppo import visit_fields
    m = np.zeros((17, 17), np.int64)
    m[2, 14], m[15, 1] = 3, 9
    vs = dict(rollout=m, other=0, cells_mean=4.5, cells_min=2, cells_max=7)
    assert visit_fields(vs) == " cells mean/min/max 4.50/2/7 room2 0.2500"
    assert visit_fields(dict(vs, cells_mean=None, cells_min=None, cells_max=None)) == " cells mean/min/max -/-/- room2 0.2500"
