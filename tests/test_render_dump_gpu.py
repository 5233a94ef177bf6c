"""train_ppo --dump_frames DIR --dump_envs K: the frames written once per update equal the numpy restatement
(tests/render_ref.py) applied to the state written beside them, and the flags change nothing else: the log lines of a run
with the flags have the fields of a run without them."""
import os
import re

import numpy as np
import pytest

import render_ref as rr

pytestmark = pytest.mark.gpu
ARGS = ["--env", "MiniGrid-twoarmy-17x17-v6", "--num_envs", "64", "--rollout_steps", "16", "--minibatch", "256",
        "--updates", "2", "--k_epochs", "1", "--her", "False", "--cuda", "cuda:0"]


def _lines(capsys):
    return [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]


def test_dumped_frames_equal_restatement_and_the_log_is_unchanged(tmp_path, capsys):
    from twoarmy_amd._lib import FIELDS
    from twoarmy_amd.soa import train_ppo
    train_ppo.main(ARGS)
    plain = _lines(capsys)
    d = str(tmp_path / "frames")
    train_ppo.main(ARGS + ["--dump_frames", d, "--dump_envs", "5", "--tile_size", "8"])
    dumped = _lines(capsys)
    assert sorted(os.listdir(d)) == ["update_0_frames.npy", "update_0_state.npz", "update_1_frames.npy",
                                     "update_1_state.npz"]
    for u in range(2):
        frames = np.load(os.path.join(d, "update_%d_frames.npy" % u))
        z = np.load(os.path.join(d, "update_%d_state.npz" % u))
        rec = z["records"]
        assert frames.shape == (5, 17 * 8, 17 * 8, 3) and frames.dtype == np.uint8 and rec.shape == (5, 48)
        ref, err = rr.render_frames(z["type"], z["colour"], None, 17, 17, rec[:, FIELDS["AX"]], rec[:, FIELDS["AY"]],
                                    rec[:, FIELDS["DIR"]], 8)
        assert not err.any() and np.array_equal(frames, ref), u
    # the same fields in the same order: the lines are equal once every number is blanked
    blank = lambda ln: re.sub(r"-?\d+(?:\.\d+)?|(?<=[ /])-(?=[ /])", "#", ln)                               # noqa: E731
    assert len(plain) == len(dumped) == 2
    assert [blank(ln) for ln in plain] == [blank(ln) for ln in dumped]
    assert plain[0].startswith("update 0: rollout ") and " score " in plain[0]
