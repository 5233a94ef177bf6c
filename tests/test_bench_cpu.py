"""bench.py pieces that do not need a GPU: the roofline accounting and the CPU-baseline leg (oracle, short sample)."""
import json
import os

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_algorithmic_bytes_match_design():
    # 2041 B per env-step + 1540 B of plane/record traffic per launch amortised over T
    assert bench.algorithmic_bytes_per_env_step(17, 128) == 2041 + 1540 / 128.0
    assert bench.algorithmic_bytes_per_env_step(7, 128) == 4 + 147 + 1156 + 8 + 4 + 1 + 1 + 1540 / 128.0
    assert bench.algorithmic_bytes_per_env_step(17, 128, 289) == 2041 - 867 + 1540 / 128.0        # uint8 code frames


def test_traffic_profile_is_only_reported_for_the_build_it_was_taken_on(tmp_path):
    alg = bench.algorithmic_bytes_per_env_step(17, 128) * 4096 * 128
    for name, bid, t in (("r07_traffic.json", "aaaa", 1.01 * alg), ("r08_traffic.json", "bbbb", 1.02 * alg),
                         ("r06_traffic.json", None, 1.5 * alg)):
        d = {"traffic_bytes_per_launch": t, "algorithmic_bytes_per_launch": alg}
        if bid:
            d["build_id"] = bid
        (tmp_path / name).write_text(json.dumps(d))
    t, src = bench.traffic_from_profile("v6", 4096, 128, 17, build_id="aaaa", profiles_dir=str(tmp_path))
    assert t == 1.01 * alg and "r07_traffic.json" in src
    t, src = bench.traffic_from_profile("v6", 4096, 128, 17, build_id="bbbb", profiles_dir=str(tmp_path))
    assert t == 1.02 * alg and "r08_traffic.json" in src
    t, src = bench.traffic_from_profile("v6", 4096, 128, 17, build_id="cccc", profiles_dir=str(tmp_path))
    assert t is None and "stale" in src and "r06_traffic.json: build not recorded" in src    # never a stale number
    assert bench.traffic_from_profile("v4", 4096, 128, 17, build_id="aaaa", profiles_dir=str(tmp_path)) == (None, None)


def test_committed_traffic_profiles_are_consistent_with_the_accounting():
    alg = bench.algorithmic_bytes_per_env_step(17, 128) * 4096 * 128
    pdir = os.path.join(ROOT, "profiles")
    names = [f for f in os.listdir(pdir) if f.endswith("_traffic.json")]
    assert names
    for name in names:
        with open(os.path.join(pdir, name)) as f:
            prof = json.load(f)
        assert abs(prof["algorithmic_bytes_per_launch"] - alg) < 1.0
        assert 0.98 * alg < prof["traffic_bytes_per_launch"] < 1.10 * alg       # measured HBM bytes: no wasted re-reads / re-writes


def test_library_reports_the_build_id_of_its_sources():
    import hashlib
    import twoarmy_amd
    twoarmy_amd._lib.build()
    csrc = twoarmy_amd._lib.CSRC_DIR
    files = [os.path.join(csrc, f) for f in ("twoarmy_engine.hip", "ppo_kernels.hip", "minigrid_view.hip")] + \
        sorted(os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    h = hashlib.sha256()
    for fn in files:
        with open(fn, "rb") as f:
            h.update(f.read())
    assert twoarmy_amd._lib.lib().tw_build_id().decode() == h.hexdigest()[:16]


def test_region_count_rule():
    assert bench.auto_regions(20, 0.17) == 295                  # the driver's command at 4096 envs: ~1 s of GPU time
    assert bench.auto_regions(20, 5.0) == 25                    # never fewer than 25 regions
    assert bench.auto_regions(4, 0.05) == 400                   # ... nor more than 400
    assert 0.9 < bench.auto_regions(40, 0.17) * 40 * 0.17 / 1000.0 < 1.1


def test_cpu_baseline_leg_runs_the_oracle():
    assert 1 <= bench.usable_cores() <= 64
    r = bench.cpu_baseline(6, 256, 17, seconds=0.5)
    assert r["kind"] == "port" and r["unit"] == "env-steps/s" and r["value"] > 1e4 and r["single_thread_value"] > 1e4
    assert r["cores"] == bench.usable_cores()


def test_plain_run_options():
    a = bench.build_parser().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and a.full is False and a.dump_outputs is None
    a = bench.build_parser().parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_zero_steps_is_refused_before_anything_runs():
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr and '"metric"' not in p.stdout


def test_dump_sample_is_fixed_and_seeded():
    import numpy as np
    a, b = bench.dump_env_sample(4096), bench.dump_env_sample(4096)
    assert np.array_equal(a, b) and len(a) == bench.DUMP_SAMPLE_ENVS == len(set(a.tolist()))
    assert np.all(np.diff(a) > 0) and 0 <= a[0] and a[-1] < 4096
    assert np.array_equal(bench.dump_env_sample(10), np.arange(10))


def test_write_outputs_float_files_and_size_limit(tmp_path):
    import numpy as np
    import pytest
    rec = bench.write_outputs(str(tmp_path / "d"), {"obs": np.arange(6, dtype=np.uint8).reshape(2, 3),
                                                    "ret": np.ones(3, np.float64)})
    assert rec["files"] == ["obs.npy", "ret.npy"] and rec["bytes"] == 6 * 4 + 3 * 8
    obs, ret = np.load(tmp_path / "d" / "obs.npy"), np.load(tmp_path / "d" / "ret.npy")
    assert obs.dtype == np.float32 and np.array_equal(obs, np.arange(6).reshape(2, 3)) and ret.dtype == np.float64
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, np.float32)})
    assert not (tmp_path / "big").exists()


def test_dump_engine_outputs_takes_the_sampled_env_columns(tmp_path):
    import numpy as np
    import torch
    T, N = 4, 300
    g = torch.Generator().manual_seed(1)
    out = {"obs": torch.randint(0, 255, (T, N, 17, 17, 3), dtype=torch.uint8, generator=g),
           "matrix": torch.rand((T, N, 289), generator=g), "pos": torch.rand((T, N, 2), generator=g),
           "reward": torch.rand((T, N), generator=g), "terminated": torch.randint(0, 2, (T, N), dtype=torch.uint8, generator=g),
           "truncated": torch.randint(0, 2, (T, N), dtype=torch.uint8, generator=g)}
    rec = bench.dump_engine_outputs(str(tmp_path), out, N, rollout=True)
    ids = bench.dump_env_sample(N)
    assert np.array_equal(np.load(tmp_path / "env_ids.npy"), ids.astype(np.float32))
    for k, t in out.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, t[:, torch.as_tensor(ids)].float().numpy()), k
    assert rec["bytes"] == sum(np.load(tmp_path / f).nbytes for f in rec["files"])
    # step launches hand back [N, ...]
    rec = bench.dump_engine_outputs(str(tmp_path / "s"), {k: t[0] for k, t in out.items()}, N, rollout=False)
    assert np.load(tmp_path / "s" / "obs.npy").shape == (len(ids), 17, 17, 3)


def test_dump_ppo_outputs_rollout_columns_and_parameters(tmp_path):
    import types
    import numpy as np
    import torch
    T, N = 8, 100
    tr = types.SimpleNamespace(N=N, action=torch.randint(0, 5, (T, N), dtype=torch.int32), logp=torch.rand(T, N),
                               reward=torch.rand(T, N), term=torch.randint(0, 2, (T, N), dtype=torch.uint8),
                               trunc=torch.randint(0, 2, (T, N), dtype=torch.uint8))
    agent = types.SimpleNamespace(actor=torch.nn.Linear(3, 2), critic=torch.nn.Linear(3, 1))
    rec = bench.dump_ppo_outputs(str(tmp_path), tr, agent)
    ids = torch.as_tensor(bench.dump_env_sample(N))
    assert np.array_equal(np.load(tmp_path / "reward.npy"), tr.reward[:, ids].numpy())
    assert np.array_equal(np.load(tmp_path / "action.npy"), tr.action[:, ids].float().numpy())
    actor = np.load(tmp_path / "actor_params.npy")
    assert actor.shape == (3 * 2 + 2,) and np.array_equal(actor[:6], agent.actor.weight.detach().reshape(-1).numpy())
    assert set(rec["files"]) == {"env_ids.npy", "action.npy", "logp.npy", "reward.npy", "terminated.npy", "truncated.npy",
                                 "actor_params.npy", "critic_params.npy"}
