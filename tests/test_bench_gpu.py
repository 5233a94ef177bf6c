"""bench.py on the GPU, driven exactly like the driver drives it: one JSON line, `value` and `roofline.achieved` from the
same timed launches, engine slab outputs; --full and --dump-outputs; and the --gpus 2 launcher on a one-GPU box (two ranks
share the GPU, gloo)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=600):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_driver_command_line():
    r = _bench(["--gpus", "1", "--steps", "6", "--warmup", "2"])
    assert r["metric"] == "env-steps/sec" and r["n_gpus"] == 1 and r["steps"] == 6 and r["warmup"] == 2
    assert r["unit"] == "env-steps/s" and r["higher_is_better"] is True and r["dtype"] == "u8" and r["ms_per_step"] > 0
    assert abs(r["value"] * r["ms_per_step"] * 1e-3 - 4096 * 128) < 1e-6 * 4096 * 128        # both from the same K steps
    assert "cpu_baseline" not in r and "regions" not in r["roofline"]                         # a plain run stays lean
    assert r["config"]["env_steps_per_step"] == 4096 * 128 and "records" in r["config"]["output_buffers"]
    rf = r["roofline"]
    assert rf["bound"] == "hbm" and rf["launches_timed"] == 6 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    # value (host wall clock) and achieved (events on the launch stream) describe the same launches
    implied = r["value"] * rf["algorithmic_bytes_per_env_step"] / 1e9
    assert 0.9 * rf["achieved"] < implied <= 1.001 * rf["achieved"]
    assert r["value"] > 1.0e9                                   # a launch-bound or fallback path would be far below


def test_full_run_keeps_every_extra_measurement():
    """--full: the same headline, then more timed regions, the slab check, the fill ceiling and the CPU baseline."""
    r = _bench(["--gpus", "1", "--steps", "6", "--warmup", "2", "--full"])
    assert r["steps"] == 6 and r["roofline"]["launches_timed"] == 6
    rf = r["roofline"]
    assert 25 <= rf["regions"] <= 400 and rf["gpu_ms_timed_total"] > 0 and rf["regions_value_median"] > 1.0e9
    assert rf["kernel_ms_samples"]["min"] <= rf["kernel_ms_samples"]["median"] <= rf["kernel_ms_samples"]["max"]
    assert rf["measured_fill_ceiling_GBs"] > 1000 and rf["frac_of_measured_fill_ceiling"] > 0
    assert len(r["config"]["slab_check_ms"]["ms"]) == 3
    cb = r["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 1e4


def test_dump_outputs_are_what_the_last_timed_launch_computed(tmp_path):
    """--dump-outputs: the sampled env columns of the last timed launch, the same in two runs and equal to W + K launches
    of a fresh engine with the same action window (the clock warm-up launches leave no trace)."""
    import numpy as np
    import torch
    import bench
    from twoarmy_amd.engine import TwoarmyEngine
    N, W, K, T = 1024, 2, 3, bench.ROLLOUT_T
    args = ["--gpus", "1", "--steps", str(K), "--warmup", str(W), "--envs", str(N), "--dump-outputs"]
    dumps = []
    for d in ("a", "b"):
        r = _bench(args + [str(tmp_path / d)])
        assert r["outputs_dumped"]["bytes"] <= 64 << 20
        files = sorted(os.listdir(tmp_path / d))
        assert files == r["outputs_dumped"]["files"]
        dumps.append({f[:-4]: np.load(tmp_path / d / f) for f in files})
    a, b = dumps
    assert set(a) == {"env_ids", "obs", "matrix", "pos", "reward", "terminated", "truncated"}
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
    ids = bench.dump_env_sample(N)
    assert np.array_equal(a["env_ids"], ids.astype(np.float32)) and len(ids) == bench.DUMP_SAMPLE_ENVS
    assert a["obs"].shape == (T, len(ids), 17, 17, 3) and a["matrix"].shape == (T, len(ids), 289)

    torch.cuda.set_device(0)
    eng = TwoarmyEngine(6, N, 17, device="cuda:0", seed=bench.SEED)
    n_act = min(W + K, 64)
    actions = eng.fill_actions(n_act * T).view(n_act, T, N)
    out = eng.alloc_outputs(T)
    for i in range(W + K):
        eng.rollout(T, out, actions=actions[i % n_act], autoreset=True, policy_idx=True)
    torch.cuda.synchronize()
    idx = torch.as_tensor(ids, device="cuda:0")
    for k in ("obs", "matrix", "pos", "reward", "terminated", "truncated"):
        assert np.array_equal(a[k], out[k][:, idx].float().cpu().numpy()), k
    eng.close()


def test_two_ranks_on_one_gpu_through_the_launcher():
    r = _bench(["--gpus", "2", "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--envs", "1024"])
    assert r["n_gpus"] == 2
    c = r["config"]["collective"]
    assert c["world_size"] == 2 and c["sanity_allreduce_of_ones"] == 2.0


def test_two_ranks_ppo_mode_zero_copy_bucket():
    """--mode ppo on two ranks (they share the GPU: gloo): every optimiser step issues two all-reduces (actor's while the
    critic's backward runs, then the critic's), nothing is copied into the bucket, the line carries the bucket's timings."""
    r = _bench(["--gpus", "2", "--mode", "ppo", "--variant", "v4", "--envs", "256", "--minibatch", "8192", "--k-epochs", "2",
                "--steps", "1", "--warmup", "1", "--graph", "off"], timeout=900)
    assert r["n_gpus"] == 2 and r["dtype"] == "f32"
    gb = r["config"]["grad_bucket"]
    steps = gb["optimiser_steps_per_iteration"]
    assert steps == 2 * 4                                        # 256 x 128 samples / 8192 per minibatch, K = 2
    assert gb["allreduces_issued"] == 2 * steps and gb["gradients_copied_into_bucket"] == 0
    assert gb["floats"] == 2515206 and gb["ms_per_allreduce"] > 0 and gb["ms_exposed_per_optimiser_step_mean"] > 0
    assert r["config"]["slab_backing"]["agree"] is True
