"""The one launch path on a device: a successful launch leaves the error state alone, a ppo_ops launch runs on its
tensors' device whichever device is current, and the name a failure would be reported under is the symbol called.
Failing launches are not provoked here (tests/test_launch_cpu.py covers the failure without a device)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _error_state():
    import twoarmy_amd
    lib = twoarmy_amd._lib.lib()
    return lib.tw_last_hip_error(), lib.tw_last_error_message()


def _rollout(T, N, seed, dev):
    """terminated, truncated u8[T,N], age0 i32[N], reward / value / next_value f32[T,N], pos f32[T,N,2] inside 17x17."""
    g = torch.Generator().manual_seed(seed)
    term = (torch.rand(T, N, generator=g) < 0.3).to(torch.uint8)
    trunc = (torch.rand(T, N, generator=g) < 0.2).to(torch.uint8)
    age0 = torch.randint(0, 5, (N,), generator=g, dtype=torch.int32)
    f = [torch.randn(T, N, generator=g) for _ in range(3)]
    pos = torch.randint(0, 17, (T, N, 2), generator=g).float()
    return [t.to(dev) for t in [term, trunc, age0] + f + [pos]]


def test_error_state_stays_clean_after_successful_launches():
    from twoarmy_amd import minigrid_nav, ppo_ops
    from twoarmy_amd.engine import TwoarmyEngine
    dev = torch.device("cuda:0")
    term, trunc, age0 = _rollout(3, 65, 1, dev)[:3]
    age = ppo_ops.age_scan(term, trunc, age0)
    dist = torch.arange(3 * 25, dtype=torch.int32, device=dev).to(torch.int16).view(minigrid_nav.DIST_DTYPE).view(3, 25)
    pos = torch.tensor([[1.0, 2.0], [0.0, 4.0], [3.0, 3.0]], device=dev)
    looked = minigrid_nav.lookup(dist, pos, 5, 5)
    eng = TwoarmyEngine(6, 64, 17, device=dev, seed=9981)
    out = eng.step(torch.zeros(64, dtype=torch.int32, device=dev), eng.alloc_outputs())
    torch.cuda.synchronize(dev)
    eng.close()
    assert age.shape == (4, 65) and looked.shape == (3,) and out["reward"].shape == (64,)
    assert minigrid_nav.as_int(looked).tolist() == [1 * 5 + 2, 25 + 0 * 5 + 4, 50 + 3 * 5 + 3]
    assert _error_state() == (0, b"")


def _follow(dev):
    """age_scan, gae and VisitTracker.account at T = 3, N = 65 (one full wavefront plus one lane) on `dev`, on the host."""
    from twoarmy_amd import ppo_ops
    from twoarmy_amd.visitation import VisitTracker
    term, trunc, age0, reward, value, next_value, pos = _rollout(3, 65, 2, dev)
    got = {"age": ppo_ops.age_scan(term, trunc, age0)}
    got["adv"], got["target"], got["ret"] = ppo_ops.gae(reward, value, next_value, term, gamma=0.99, lam=0.95,
                                                        use_done_mask=True)
    tracker = VisitTracker(65, dev)
    tracker.account(pos, term, trunc)
    got.update(first_visit=tracker.first_visit, ep_cells=tracker.ep_cells, maps=tracker._buf, carry=tracker.carry)
    assert all(t.device == torch.device(dev) for t in got.values())
    return {k: t.cpu() for k, t in got.items()}


def test_launches_follow_their_tensors_to_another_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    torch.cuda.set_device(0)
    want = _follow("cuda:0")
    got = _follow("cuda:1")                    # the current device stays cuda:0
    assert torch.cuda.current_device() == 0
    assert want["maps"][:290].sum() == 3 * 65
    for k in want:
        assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), k
    assert _error_state() == (0, b"")


def test_failures_would_be_reported_under_the_symbol_called(monkeypatch):
    import twoarmy_amd
    from twoarmy_amd import ppo_ops
    dev = torch.device("cuda:0")
    names, check = [], twoarmy_amd._lib.check

    def recorder(rc, what):
        names.append(what)
        check(rc, what)

    K, N, B = 4, 3, 5
    frames = torch.randint(0, 4, (K, N, 304), dtype=torch.uint8, device=dev)[..., :289]
    # (k, n, age) of each record; slot j of a record reads frame k - (3 - j) while age > 3 - j, so age <= k + 1
    idx = [torch.tensor(v, dtype=torch.int32, device=dev) for v in ([3, 0, 2, 3, 1], [0, 1, 2, 2, 0], [4, 1, 0, 2, 2])]
    init_frame = torch.full((289,), 0.25, device=dev)
    probs = torch.full((7, 5), 0.2, device=dev)
    offset_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    monkeypatch.setattr(twoarmy_amd._lib, "check", recorder)
    out, pos_out = ppo_ops.gather_stack(frames, None, *idx, init_frame, None)
    action, logp = ppo_ops.sample(probs, None, seed=3, offset=0, offset_dev=offset_dev)
    monkeypatch.undo()
    torch.cuda.synchronize(dev)
    assert names == ["ppo_gather_stack_u8", "ppo_sample_dev"]
    assert out.shape == (B, 4, 289) and pos_out is None
    lut = torch.tensor([0.9, -0.9, -0.5, 0.3], device=dev)
    assert torch.equal(out[0], lut[frames[:, 0].long()]) and bool((out[2] == 0.25).all())
    assert action.shape == (7,) and bool(((action >= 0) & (action < 5)).all()) and bool(torch.isfinite(logp).all())
