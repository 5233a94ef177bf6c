"""_marshal.agent_arrays and the observation front ends that read the agent through it: column views of a record tensor
give exactly what contiguous copies of the same values give, and arrays the C ABI cannot describe with one stride are
rejected by assertion before anything is launched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = H = 5


def _world(N, seed):
    """Planes with walls, a goal per env and doors with a state, and records that hold the agent among other words."""
    from twoarmy_amd._lib import TW_REC_WORDS
    rs = np.random.RandomState(seed)
    ty = rs.choice(np.array([1, 1, 1, 2, 4, 5], np.uint8), (N, W * H))
    ty[np.arange(N), rs.randint(0, W * H, N)] = 8
    co = rs.randint(0, 6, (N, W * H)).astype(np.uint8)
    st = rs.randint(0, 3, (N, W * H)).astype(np.uint8)
    rec = rs.randint(-9999, 9999, (N, TW_REC_WORDS)).astype(np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2] = rs.randint(0, W, N), rs.randint(0, H, N), rs.randint(0, 4, N)
    rec[N - 1, 0] = W                                            # one agent outside the world: error 2 on both paths
    return [torch.from_numpy(a).to(DEV) for a in (ty, co, st, rec)]


@pytest.mark.parametrize("N", [3, 1])
def test_record_columns_give_what_contiguous_copies_give(N):
    from twoarmy_amd import minigrid_obs as mo
    from twoarmy_amd._lib import TW_REC_WORDS
    from twoarmy_amd._marshal import agent_arrays
    ty, co, st, rec = _world(N, 11 + N)
    cols = [rec[:, k] for k in range(3)]
    dense = [c.contiguous() for c in cols]
    # the stride comes from the tensors; a single row has none to show and reads as stride 1
    assert agent_arrays(*cols)[3] == (TW_REC_WORDS if N > 1 else 1) and agent_arrays(*dense)[3] == 1
    assert [p.value for p in agent_arrays(*cols)[:3]] == [rec.data_ptr() + 4 * k for k in range(3)]
    assert agent_arrays(cols[0], cols[1])[2] is None
    full_c, err_c = mo.full_obs(ty, co, st, W, H, *cols, want_error=True)
    full_d, err_d = mo.full_obs(ty, co, st, W, H, *dense, want_error=True)
    assert torch.equal(full_c, full_d) and torch.equal(err_c, err_d)
    assert err_d.tolist() == [0] * (N - 1) + [2]
    ax, ay, ad = (t.cpu().numpy() for t in dense)
    got = full_d.cpu().numpy()
    for e in range(N - 1):                                       # and the agent was read at all: its cell carries it
        assert got[e, ax[e], ay[e]].tolist() == [10, 0, ad[e]]
    k = mo.goal_index(ty, W, H)
    tab = mo.angle_table(W, H, DEV)
    for mode in ("slope", "angle"):
        dir_c, e_c = mo.goal_direction(k, W, H, cols[0], cols[1], mode=mode, table=tab, want_error=True)
        dir_d, e_d = mo.goal_direction(k, W, H, dense[0], dense[1], mode=mode, table=tab, want_error=True)
        assert torch.equal(dir_c.view(torch.int64), dir_d.view(torch.int64)) and torch.equal(e_c, e_d)   # bits: NaN as NaN
        assert e_d.tolist() == [0] * (N - 1) + [2]


def test_arrays_without_one_stride_are_rejected_before_any_launch():
    from twoarmy_amd import minigrid_obs as mo
    from twoarmy_amd._marshal import agent_arrays
    N = 3
    ty, co, st, rec = _world(N, 5)
    cols = [rec[:, k] for k in range(3)]
    dense = [c.contiguous() for c in cols]
    bad = [
        (cols[0], dense[1], cols[2]),                            # mixed strides
        (dense[0], dense[1], cols[2]),
        (dense[0], dense[1].long(), dense[2]),                   # not int32
        (dense[0].cpu(), dense[1], dense[2]),                    # a host tensor
        (dense[0], dense[1], dense[2].cpu()),
        (dense[0], dense[1][:2], dense[2]),                      # lengths differ
        (rec[:, :1], rec[:, 1:2], rec[:, 2:3]),                  # not 1-D
        tuple(d[:1].expand(N) for d in dense),                   # one stride, but not a positive one
    ]
    out = torch.full((N, W, H, 3), 0xA5, dtype=torch.uint8, device=DEV)
    for args in bad:
        with pytest.raises(AssertionError):
            agent_arrays(*args)
        with pytest.raises(AssertionError):
            mo.full_obs(ty, co, st, W, H, *args, out=out)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())                             # nothing was launched
    mo.full_obs(ty, co, st, W, H, *cols, out=out)
    assert not bool((out == 0xA5).all())
