"""Visit counting on the MI355X: ppo_visit_scan / ppo_visit_hist against the numpy restatement (tests/visit_ref.py), on
the reference's recorded buffers and traces, and through VisitTracker, VecPPOTrainer, TwoarmyVecEnv and
train_ppo --visit_dir.  Every comparison is exact integer equality."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import visit_ref as VR
from golden_util import load_traces

pytestmark = pytest.mark.gpu
_, SEED = load_traces()
DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def carry_dev(seen, W, H):
    return dev(VR.sets_to_carry(seen, W, H).view(np.int32))


def scan_in_cuts(pos, term, trunc, cuts, seen0, W, H, want_steps=True):
    """ppo_ops.visit_scan over consecutive launches of the given lengths -> host (first_visit, ep_cells, carry words)."""
    from twoarmy_amd import ppo_ops
    assert sum(cuts) == pos.shape[0]
    carry = carry_dev(seen0, W, H)
    pd, td, ud = dev(pos), dev(term), dev(trunc)
    firsts, cells, t = [], [], 0
    for c in cuts:
        a, b = ppo_ops.visit_scan(pd[t:t + c], td[t:t + c], ud[t:t + c], carry, W, H, want_steps=want_steps)
        if want_steps:
            firsts.append(a.cpu().numpy()); cells.append(b.cpu().numpy())
        else:
            assert a is None and b is None
        t += c
    return (np.concatenate(firsts) if firsts else None, np.concatenate(cells) if cells else None,
            carry.cpu().numpy().view(np.uint32))


def hist_dev(pos, W, H, counts=None, **kw):
    from twoarmy_amd import ppo_ops
    counts = torch.zeros(W * H + 1, dtype=torch.int64, device=DEV) if counts is None else counts
    kw = {k: (None if v is None else dev(v)) for k, v in kw.items()}
    return ppo_ops.visit_hist(dev(pos), counts, W, H, **kw).cpu().numpy()


def walks(T, N, W, H, seed, p_done=0.05):
    """Random walks on the grid with resets to one start cell, like the engine's episodes."""
    rng = np.random.default_rng(seed)
    moves = np.array([[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1]])
    done = rng.random((T, N)) < p_done
    term = (done & (rng.random((T, N)) < 0.5)).astype(np.uint8)
    trunc = (done & (term == 0)).astype(np.uint8)
    pos = np.empty((T, N, 2), np.float32)
    cur = np.tile(np.array([H - 2, 1]), (N, 1)) if H > 2 and W > 1 else np.zeros((N, 2), np.int64)
    start = cur.copy()
    for t in range(T):
        cur = np.clip(cur + moves[rng.integers(0, 5, N)], 0, [H - 1, W - 1])
        pos[t] = cur
        cur = np.where(done[t][:, None], start, cur)
    seen0 = [set(rng.integers(0, W * H, rng.integers(1, 6)).tolist()) for _ in range(N)]
    return pos, term, trunc, seen0


def check_scan(pos, term, trunc, seen0, W, H, cuts):
    want_first, want_cells, want_seen = VR.visit_scan(pos, term, trunc, W, H, seen0)
    first, cells, carry = scan_in_cuts(pos, term, trunc, cuts, seen0, W, H)
    assert np.array_equal(first, want_first), cuts[:4]
    assert np.array_equal(cells, want_cells), cuts[:4]
    assert np.array_equal(carry, VR.sets_to_carry(want_seen, W, H)), cuts[:4]
    return want_first, want_cells, carry


# ------------------------------------------------------------------ recorded data
def test_hist_on_the_reference_buffers_dense_and_indexed():
    rng = np.random.default_rng(0)
    for name, p in VR.her_buffers():
        pos = p.reshape(-1, 1, 2)
        ref = VR.reference_heatmap(p).astype(np.int64)                   # heatmap.py:58-63, literally
        got = hist_dev(pos, 17, 17)
        assert got[289] == 0 and np.array_equal(got[:289].reshape(17, 17), ref), name
        idx = rng.integers(0, len(p), 3 * len(p) // 2).astype(np.int32)   # shuffled, with duplicates
        zeros = np.zeros_like(idx)
        got = hist_dev(pos, 17, 17, t_idx=idx, n_idx=zeros)
        assert np.array_equal(got, VR.visit_hist(pos, 17, 17, t_idx=idx, n_idx=zeros)), name
        assert len(np.unique(idx)) < len(idx) and got.sum() == len(idx)


def test_scan_on_recorded_traces_in_unequal_cuts():
    for variant, columns in VR.golden_columns().items():
        pos, term, trunc = VR.stacked(columns)
        T, N = term.shape
        assert (T, N) == ((160, 6) if variant == 6 else (200, 10))
        cuts = [64, 64, 32] if T == 160 else [64, 64, 32, 40]
        first, cells, _ = check_scan(pos, term, trunc, [set()] * N, 17, 17, cuts)
        n_eps = 0
        for n, (p, te, tu) in enumerate(columns):                        # against np.unique per episode (env_buffer.py:138)
            start = 0
            for t in np.nonzero(te | tu)[0].tolist():
                index, n_unique = VR.reference_goal_candidates(p[start:t + 1])
                assert np.nonzero(first[start:t + 1, n])[0].tolist() == index and cells[t, n] == n_unique
                start = t + 1
                n_eps += 1
        assert n_eps == (18 if variant == 6 else 40)
        mask = (term | trunc)
        assert np.array_equal(hist_dev(pos, 17, 17, mask=mask), VR.visit_hist(pos, 17, 17, mask=mask))


# ------------------------------------------------------------------ cut invariance
@pytest.mark.parametrize("N", [1000, 5])
def test_scan_is_invariant_under_the_cut(N):
    T = 300
    pos, term, trunc, seen0 = walks(T, N, 17, 17, 11 + N)
    assert all(seen0) and (term | trunc).sum() > T * N // 40
    want = None
    for cuts in ([T], [1] * T, [7, 64, 128, 101]):
        got = check_scan(pos, term, trunc, seen0, 17, 17, cuts)
        bare = scan_in_cuts(pos, term, trunc, cuts, seen0, 17, 17, want_steps=False)   # nullable outputs: the carry alone
        assert bare[0] is None and np.array_equal(bare[2], got[2])
        want = got if want is None else want
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    full = hist_dev(pos, 17, 17)
    assert np.array_equal(full, VR.visit_hist(pos, 17, 17)) and full.sum() == T * N
    assert np.array_equal(hist_dev(pos, 17, 17, mask=want[0]), VR.visit_hist(pos, 17, 17, mask=want[0]))


# ------------------------------------------------------------------ contention
def test_hist_with_every_env_on_one_cell():
    T, N = 3, 4096
    pos = np.empty((T, N, 2), np.float32)
    pos[..., 0], pos[..., 1] = 15.0, 1.0
    got = hist_dev(pos, 17, 17)
    assert got[15 * 17 + 1] == T * N and got.sum() == T * N
    none = np.zeros((T, N), np.uint8)
    first, cells, _ = check_scan(pos, none, none, [set()] * N, 17, 17, [T])
    assert first[0].all() and not first[1:].any() and (cells == 1).all()


def test_hist_with_every_env_on_its_own_cell_and_a_64_bit_accumulate():
    N = 289
    cell = np.random.default_rng(1).permutation(N)
    pos = np.stack([cell // 17, cell % 17], 1).astype(np.float32).reshape(1, N, 2)
    got = hist_dev(pos, 17, 17)
    assert got[:289].tolist() == [1] * 289 and got[289] == 0
    pre = (2 ** 40 + np.arange(290)).astype(np.int64)
    pre[7] = 2 ** 32 - 1                                                 # the add carries into the high word
    got = hist_dev(np.repeat(pos, 3, 0), 17, 17, counts=dev(pre))
    assert np.array_equal(got, pre + np.array([3] * 289 + [0]))


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_env_counts_around_the_wavefront(N):
    T = 21
    pos, term, trunc, seen0 = walks(T, N, 17, 17, N, p_done=0.1)
    first, _, _ = check_scan(pos, term, trunc, seen0, 17, 17, [T])
    assert np.array_equal(hist_dev(pos, 17, 17, mask=first), VR.visit_hist(pos, 17, 17, mask=first))
    got = check_scan(pos[:1], term[:1], trunc[:1], seen0, 17, 17, [1])   # T = 1
    assert np.array_equal(hist_dev(pos[:1], 17, 17), VR.visit_hist(pos[:1], 17, 17)) and got[0].shape == (1, N)


@pytest.mark.parametrize("W,H", [(1, 1), (5, 9), (9, 5), (32, 32)])
def test_grid_shapes(W, H):
    from twoarmy_amd import ppo_ops
    T, N = 90, 70
    assert ppo_ops.visit_carry_words(W, H, N) == (W * H + 31) // 32 * N
    pos, term, trunc, seen0 = walks(T, N, W, H, W * 100 + H)
    pos[3, 5] = (H, 0); pos[4, 6] = (0, W); pos[5, 7] = (H - 1, W - 1)   # just outside, and the last cell
    check_scan(pos, term, trunc, seen0, W, H, [50, 40])
    got = hist_dev(pos, W, H)
    assert np.array_equal(got, VR.visit_hist(pos, W, H)) and got[W * H] >= 2 and got.sum() == T * N
    if (W, H) == (32, 32):                                               # every bit of the largest carry
        everywhere = np.stack(np.divmod(np.arange(1024), 32), 1).astype(np.float32).reshape(1024, 1, 2)
        none = np.zeros((1024, 1), np.uint8)
        first, cells, carry = check_scan(everywhere, none, none, [set()], 32, 32, [1000, 24])
        assert first.all() and cells[-1, 0] == 1024 and (carry == 0xFFFFFFFF).all()


# ------------------------------------------------------------------ edges
def test_positions_outside_the_grid():
    W, H = 9, 5
    bad = [np.nan, np.inf, -np.inf, -1.0, float(H), float(W), 1e9, -1e-30, 32.0, 2.0 ** 31, -2.0 ** 31]
    rows = [(b, 1.0) for b in bad] + [(1.0, b) for b in bad]
    rows = [r for r in rows if VR.cell_of(r[0], r[1], W, H) == W * H]        # (1, 5.0) is inside: x = height < width
    assert len(rows) >= 18
    T = len(rows) + 2
    pos = np.ones((T, 2, 2), np.float32)
    pos[1:-1, 0] = np.array(rows, np.float32)
    none = np.zeros((T, 2), np.uint8)
    first, cells, carry = check_scan(pos, none, none, [set(), set()], W, H, [T])
    assert first[:, 0].tolist() == [1] + [0] * (T - 1) and (cells == 1).all()      # no bit set, no first visit
    assert VR.carry_to_sets(carry, 2, W, H) == [{W + 1}, {W + 1}]
    got = hist_dev(pos, W, H)
    assert got[W * H] == len(rows) and got[W + 1] == 2 * T - len(rows) and got.sum() == 2 * T
    # -0.0 satisfies 0 <= y as a float comparison and int(-0.0) = 0: cell 0, like values_matrix[int(-0.0), int(-0.0)]
    zero = np.full((1, 1, 2), -0.0, np.float32)
    assert hist_dev(zero, W, H)[0] == 1
    assert check_scan(zero, none[:1, :1], none[:1, :1], [set()], W, H, [1])[0][0, 0] == 1


def test_done_on_the_first_and_the_last_step():
    T, N = 12, 66
    pos, _, _, seen0 = walks(T, N, 17, 17, 3)
    term = np.zeros((T, N), np.uint8); trunc = np.zeros((T, N), np.uint8)
    term[0, ::2], trunc[0, 1::3], trunc[T - 1, :] = 1, 1, 1
    _, cells, carry = check_scan(pos, term, trunc, seen0, 17, 17, [T])
    assert not carry.any()                                              # every episode ended with the rollout
    assert (cells[1, ::2] == 1).all()                                    # the step after a done starts from the empty set


def padded(shape, dtype):
    """A tensor embedded in a 0xA5-filled buffer, 64 bytes of margin on each side."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[64:64 + n].view(dtype).view(*shape)


def margins_untouched(buf):
    host = buf.cpu().numpy()
    return (host[:64] == 0xA5).all() and (host[-64:] == 0xA5).all()


def test_nullable_outputs_and_no_write_outside_the_arrays():
    from twoarmy_amd import _lib
    lib = _lib.lib()
    T, N, W, H = 9, 67, 17, 17
    pos, term, trunc, seen0 = walks(T, N, W, H, 8, p_done=0.2)
    pos[2, 3] = (np.nan, 1.0)
    want_first, want_cells, want_seen = VR.visit_scan(pos, term, trunc, W, H, seen0)
    pd, td, ud = dev(pos), dev(term), dev(trunc)
    words = VR.sets_to_carry(seen0, W, H).view(np.int32)
    for with_first, with_cells in ((True, True), (True, False), (False, True), (False, False)):
        bf, first = padded((T, N), torch.uint8)
        bc, cells = padded((T, N), torch.int32)
        bk, carry = padded((len(words),), torch.int32)
        carry.copy_(dev(words))
        rc = lib.ppo_visit_scan(ptr(pd), ptr(td), ptr(ud), T, N, W, H, ptr(carry), ptr(first) if with_first else None,
                                ptr(cells) if with_cells else None, stream())
        assert rc == 0
        assert np.array_equal(carry.cpu().numpy().view(np.uint32), VR.sets_to_carry(want_seen, W, H))
        if with_first:
            assert np.array_equal(first.cpu().numpy(), want_first)
        else:
            assert (bf.cpu().numpy() == 0xA5).all()
        if with_cells:
            assert np.array_equal(cells.cpu().numpy(), want_cells)
        else:
            assert (bc.cpu().numpy() == 0xA5).all()
        assert margins_untouched(bf) and margins_untouched(bc) and margins_untouched(bk)
    # hist: mask NULL / given, indexed with B = 0 and with records out of range; counts inside a guarded buffer
    t_idx = np.array([0, T - 1, T, -1, 2, 2, 0, 2 ** 31 - 1], np.int32)
    n_idx = np.array([0, N - 1, 0, 0, N, -1, 5, 0], np.int32)
    for kw, want in ((dict(), VR.visit_hist(pos, W, H)), (dict(mask=want_first), VR.visit_hist(pos, W, H, mask=want_first)),
                     (dict(t_idx=t_idx, n_idx=n_idx), VR.visit_hist(pos, W, H, t_idx=t_idx, n_idx=n_idx))):
        bh, counts = padded((W * H + 1,), torch.int64)
        counts.zero_()
        m, ti, ni = (None if kw.get(k) is None else dev(kw[k]) for k in ("mask", "t_idx", "n_idx"))
        rc = lib.ppo_visit_hist(ptr(pd), T, N, ptr(m), ptr(ti), ptr(ni), 0 if ti is None else len(t_idx), W, H, ptr(counts),
                                stream())
        assert rc == 0 and np.array_equal(counts.cpu().numpy(), want) and margins_untouched(bh)
    assert want[W * H] == 5 and want.sum() == 8                          # five of the eight records are out of range
    bh, counts = padded((W * H + 1,), torch.int64)
    ti = dev(t_idx)
    assert lib.ppo_visit_hist(ptr(pd), T, N, None, ptr(ti), ptr(ti), 0, W, H, ptr(counts), stream()) == 0   # B = 0
    assert (bh.cpu().numpy() == 0xA5).all()
    assert lib.ppo_visit_hist(ptr(pd), T, N, None, ptr(ti), None, 3, W, H, ptr(counts), stream()) < 0
    assert lib.ppo_visit_scan(ptr(pd), ptr(td), ptr(ud), T, N, 33, H, ptr(carry), None, None, stream()) < 0


# ------------------------------------------------------------------ front ends
def test_tracker_over_two_rollouts_is_the_restatement_over_their_concatenation():
    from twoarmy_amd.visitation import VisitTracker
    T, N = 40, 130
    pos, term, trunc, _ = walks(2 * T, N, 17, 17, 17, p_done=0.04)
    pos[5, 9] = (-1.0, 3.0)
    tr = VisitTracker(N, DEV)
    first, cells, _ = VR.visit_scan(pos, term, trunc, 17, 17)
    done = term | trunc
    got_first, got_cells, reads = [], [], []
    for k in range(2):
        sl = slice(k * T, (k + 1) * T)
        tr.account(dev(pos[sl]), dev(term[sl]), dev(trunc[sl]))
        got_first.append(tr.first_visit.cpu().numpy()); got_cells.append(tr.ep_cells.cpu().numpy())
        reads.append(tr.read())
    assert np.array_equal(np.concatenate(got_first), first) and np.array_equal(np.concatenate(got_cells), cells)
    for k, out in enumerate(reads):
        sl = slice(k * T, (k + 1) * T)
        for name, mask in (("rollout", None), ("first_visit_map", first[sl]), ("terminal_map", done[sl])):
            want = VR.visit_hist(pos[sl], 17, 17, mask=mask)
            assert out[name].shape == (17, 17) and out[name].dtype == np.int64
            assert np.array_equal(out[name].reshape(-1), want[:289]) and out["other_by_map"][name] == want[289], name
        ended = cells[sl][done[sl] != 0]
        assert out["episodes"] == len(ended) > 0
        assert out["cells_min"] == ended.min() and out["cells_max"] == ended.max()
        assert out["cells_mean"] == ended.sum() / len(ended)
    whole = VR.visit_hist(pos, 17, 17)
    assert np.array_equal(reads[1]["cumulative"].reshape(-1), whole[:289]) and reads[1]["other_by_map"]["cumulative"] == 1
    assert reads[0]["other"] == 1 and reads[1]["other"] == 0
    none = np.zeros((T, N), np.uint8)
    tr.account(dev(pos[:T]), dev(none), dev(none))                        # no finished episode
    out = tr.read()
    assert out["episodes"] == 0 and out["cells_mean"] is None and out["cells_min"] is None and out["cells_max"] is None
    tr.reset()
    assert not tr.carry.any()
    tr.account(dev(pos[0]), dev(term[0]), dev(trunc[0]))                  # one step: [N,2], [N]
    assert tr.first_visit.shape == (1, N) and tr.first_visit.all()


def test_trainer_counts_the_rollout_and_its_hindsight_records():
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    N, T = 64, 16
    torch.manual_seed(9981)
    eng = TwoarmyEngine(4, N, 17, seed=SEED)
    agent = PPO()
    agent.to(eng.device).use_nhwc()
    tr = VecPPOTrainer(agent, eng, rollout_steps=T, minibatch=256)
    with pytest.raises(RuntimeError):
        tr.visit_stats()
    seen, n_her, cumulative = None, 0, np.zeros(290, np.int64)
    for _ in range(5):
        tr.collect()
        her = tr.relabel()
        tr.account_visits(her)
        pos, term, trunc = (x.cpu().numpy() for x in (tr.pos[4:4 + T], tr.term, tr.trunc))
        ht, hn = her["t"].cpu().numpy(), her["n"].cpu().numpy()
        first, cells, seen = VR.visit_scan(pos, term, trunc, 17, 17, seen)
        want = VR.visit_hist(pos, 17, 17, t_idx=ht, n_idx=hn, counts=VR.visit_hist(pos, 17, 17))
        cumulative += want
        vs = tr.visit_stats()
        assert np.array_equal(vs["rollout"].reshape(-1), want[:289]) and vs["other"] == want[289]
        assert vs["rollout"].sum() + vs["other"] == T * N + len(ht)
        assert np.array_equal(vs["first_visit_map"].reshape(-1), VR.visit_hist(pos, 17, 17, mask=first)[:289])
        assert np.array_equal(vs["terminal_map"].reshape(-1), VR.visit_hist(pos, 17, 17, mask=term | trunc)[:289])
        assert np.array_equal(vs["cumulative"].reshape(-1), cumulative[:289])
        assert np.array_equal(tr.visits.ep_cells.cpu().numpy(), cells)
        n_her += len(ht)
        tr.carry_over()
    assert n_her > 0                                                     # max_steps = 50 < 5 * 16: every env finished
    eng.close()


def test_vecenv_records_visitation():
    from twoarmy_amd import ppo_ops
    from twoarmy_amd.vecenv import TwoarmyVecEnv
    N, S = 8, 60
    env = TwoarmyVecEnv("MiniGrid-twoarmy-17x17-v4", num_envs=N, seed=SEED, record_visitation=True)
    env.reset()
    g = torch.Generator(device="cpu").manual_seed(4)
    pos, term, trunc, cells, first = [], [], [], [], []
    for _ in range(S):
        _, _, te, tu, info = env.step(torch.randint(0, 5, (N,), generator=g))
        assert info["visitation"]["cells"].dtype == torch.int32 and info["visitation"]["first_visit"].dtype == torch.bool
        assert torch.equal(info["_visitation"], te | tu)
        pos.append(env.agent_yx.clone()); term.append(te.to(torch.uint8)); trunc.append(tu.to(torch.uint8))
        cells.append(info["visitation"]["cells"].clone()); first.append(info["visitation"]["first_visit"].clone())
    pos, term, trunc = torch.stack(pos), torch.stack(term), torch.stack(trunc)
    carry = torch.zeros(ppo_ops.visit_carry_words(17, 17, N), dtype=torch.int32, device=DEV)
    want_first, want_cells = ppo_ops.visit_scan(pos, term, trunc, carry, 17, 17)
    assert torch.equal(torch.stack(cells), want_cells) and torch.equal(torch.stack(first), want_first.bool())
    assert torch.equal(env.visit_tracker.carry, carry) and (term | trunc).sum() >= N
    ref = VR.visit_scan(pos.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), 17, 17)
    assert np.array_equal(want_cells.cpu().numpy(), ref[1])
    env.reset()
    assert not env.visit_tracker.carry.any()
    env.close()
    plain = TwoarmyVecEnv("MiniGrid-twoarmy-17x17-v4", num_envs=N, seed=SEED)
    plain.reset()
    info = plain.step(torch.zeros(N, dtype=torch.int64))[4]
    assert sorted(info) == ["_final_observation", "final_observation"] and plain.visit_tracker is None
    plain.close()


ENTRY_ARGS = ["--env", "MiniGrid-twoarmy-17x17-v4", "--num_envs", "64", "--rollout_steps", "16", "--minibatch", "256",
              "--updates", "2", "--k_epochs", "1", "--cuda", "cuda:0"]


def test_train_ppo_writes_the_maps_only_with_the_flag(tmp_path, monkeypatch, capsys):
    import re
    from twoarmy_amd.soa import train_ppo
    monkeypatch.chdir(tmp_path)
    vdir, tdir = tmp_path / "visits", tmp_path / "track"
    tr = train_ppo.main(ENTRY_ARGS + ["--visit_dir", str(vdir), "--track_buffer_file", str(tdir), "--dump_envs", "3"])
    with_flag = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]
    files = sorted(os.listdir(vdir))
    assert files == ["visits_000000_rank0.npz", "visits_000001_rank0.npz"]
    z = [np.load(vdir / f) for f in files]
    for f in z:
        assert sorted(f.files) == ["cumulative", "first_visit_map", "other", "rollout", "terminal_map"]
        assert f["rollout"].shape == (17, 17) and f["rollout"].dtype == np.int64
        assert f["rollout"].sum() + int(f["other"]) >= 16 * 64 and int(f["other"]) == 0
        assert 0 < f["first_visit_map"].sum() <= 16 * 64
    assert np.array_equal(z[0]["cumulative"], z[0]["rollout"])
    assert np.array_equal(z[1]["cumulative"], z[0]["rollout"] + z[1]["rollout"])
    assert np.array_equal(tr.visit_stats()["rollout"], z[1]["rollout"])
    tracks = sorted(os.listdir(tdir))
    assert tracks == ["track_000000.npy", "track_000001.npy"]
    track = np.load(tdir / tracks[1])
    assert track.shape == (16, 3, 2) and track.dtype == np.float64
    tail = r" cells mean/min/max (?:\d+\.\d\d/\d+/\d+|-/-/-) room2 \d\.\d{4}$"
    assert len(with_flag) == 2 and all(re.search(r"rewards \[[^\]]*\]" + tail, ln) for ln in with_flag), with_flag
    tr2 = train_ppo.main(ENTRY_ARGS)
    without = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]
    assert tr2.visits is None and len(without) == 2 and all(ln.endswith("]") and " cells " not in ln for ln in without)
    assert not glob.glob(str(tmp_path / "**" / "visits_*"), recursive=True)[2:]          # only the two written above
    assert not glob.glob(str(tmp_path / "**" / "track_*"), recursive=True)[2:]
