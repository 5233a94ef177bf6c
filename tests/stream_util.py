"""The protocol of tests/test_streams_gpu.py, written once: a case table entry, the sentinel fill, the calibrated delay,
the eager run on a side stream behind that delay (part A) and the captured, twice-replayed run (part B).  A plain
module like nav_util.py; the cases themselves live in the test file."""
import numpy as np
import torch

DEV = "cuda:0"
DELAY_MS = 40.0                       # DESIGN.md "Streams and capture": 45x the slowest measured enqueue (0.89 ms)
_cycles_per_ms = []
ENQUEUE_MS = {}                       # case name -> host time of the enqueue of its part-A run (printed by the module)


class Case:
    """One entry point reached through its front end.
    fns: the C functions the call launches.  make(seed) -> {name: device tensor}: the inputs and the in-place state of
    one valid input set (seed 0 is the decoy; every seed gives the same shapes).  outs() -> {name: tensor}: outputs and
    workspaces the caller provides (sentinel-filled by the protocol).  call(b, o, ctx) -> {name: tensor}: the results
    (new tensors, entries of o, in-place state of b).  ref(h) -> {name: array}: the CPU restatement on the host copies h
    of b before the call, None: the case compares with the default-stream run only (`note` says so).  state: names in b
    that the call updates in place and carries (part B keeps them across warm-up and replays).  tol: {name: (rtol,
    atol)} of the existing test of that op, exact where absent; ref may also return "_atol": {name: bound} where that test's
    bound depends on the data.  ref_in_b=False: part B compares with the eager sequence only.  setup(seed) -> ctx: host-side objects a run needs
    (an engine), made before the protocol starts.  blocks_host: the call returns only when its work is done.
    read(name, array) -> array: how a result or a state input is read before it meets the CPU restatement, where its
    words hold more than the restatement defines (None: as it is).
    also(part, x, y): what this case asserts beyond the protocol, called after the generic checks of each part, None:
    nothing.  Part "A": x = the side-stream results, y = the default-stream results of the decoy (seed 0), which the case
    expects to differ.  Part "B": x, y = the results of replay 1 and replay 2."""

    def __init__(self, name, family, fns, make, call, outs=None, ref=None, state=(), tol=None, setup=None, note=None,
                 exempt_b=None, blocks_host=False, ref_in_b=True, also=None, read=None):
        self.name, self.family, self.fns, self.make, self.call = name, family, tuple(fns), make, call
        self.outs, self.ref, self.state, self.tol = outs or (lambda: {}), ref, tuple(state), tol or {}
        self.setup, self.exempt_b, self.blocks_host = setup or (lambda seed: None), exempt_b, blocks_host
        self.ref_in_b, self.also, self.read = ref_in_b, also, read or (lambda name, array: array)
        self.note = note if note is not None else ("CPU restatement + default-stream run" if ref else
                                                   "default-stream run only")
        assert ref is not None or "only" in self.note

    def __repr__(self):
        return self.name


def rng(seed, salt=0):
    return np.random.default_rng(7919 * (seed + 1) + salt)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(device=DEV, dtype=dtype)


def host(t):
    return t.detach().cpu().numpy()


def raw(a):
    """The bytes of an array: equality of these is bit equality, a NaN equal to the same NaN."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


def sentinel_(t):
    """NaN for floats, 0xAB bytes for integers."""
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        assert t.is_contiguous()
        t.view(-1).view(torch.uint8).fill_(0xAB)
    return t


def sentinels(case):
    return {k: sentinel_(t) for k, t in case.outs().items()}


def delay_cycles():
    """torch.cuda._sleep cycles that keep a stream busy for DELAY_MS, measured once per process with two events."""
    if not _cycles_per_ms:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(20_000_000)
        b.record()
        torch.cuda.synchronize()
        _cycles_per_ms.append(20_000_000 / max(a.elapsed_time(b), 1e-3))
    return int(DELAY_MS * _cycles_per_ms[0])


_side = []


def side_stream():
    """A side stream whose work does not queue behind the null stream's or in front of it.  Streams share a few hardware
    queues, and two streams on one queue run in the order of submission: a launch on the wrong stream would then still
    see the staged inputs.  So a candidate is probed once: with a delay running on it, a tiny op on the null stream must
    finish first.  The stream found is kept for the whole process."""
    if not _side:
        probe = torch.zeros(1, device=DEV)
        for _ in range(16):
            s = torch.cuda.Stream()
            cycles = delay_cycles()
            torch.cuda.synchronize()
            behind, ahead = torch.cuda.Event(), torch.cuda.Event()
            with torch.cuda.stream(s):
                torch.cuda._sleep(cycles)
                behind.record(s)
            probe.add_(1)
            ahead.record(torch.cuda.default_stream())
            ahead.synchronize()
            independent = not behind.query()
            torch.cuda.synchronize()
            if independent:
                _side.append(s)
                break
        assert _side, "no side stream runs independently of the null stream"
    return _side[0]


def hip_error():
    from twoarmy_amd import _lib
    return _lib.lib().tw_last_hip_error()


def host_results(res):
    return {k: host(v) for k, v in res.items() if v is not None}


def close(ctx):
    """Free what setup() made (an engine, first in its tuple)."""
    if ctx is not None:
        ctx[0].close()


def run_default(case, seed):
    """The call on the default stream from fresh copies -> host results."""
    ctx = case.setup(seed)
    b, o = case.make(seed), sentinels(case)
    res = case.call(b, o, ctx)
    torch.cuda.synchronize()
    got = host_results(res)
    close(ctx)
    return got


def run_side(case, seed, call_on_default=False):
    """Part A, steps 1-8 -> (host results, the delay was still running when the host had enqueued everything).
    call_on_default: the controls' deliberate mistake, the call made under the default stream."""
    import time
    ctx = case.setup(seed)
    b, staging, o = case.make(0), case.make(seed), sentinels(case)
    assert set(b) == set(staging) and all(b[k].shape == staging[k].shape and b[k].dtype == staging[k].dtype for k in b)
    cycles = delay_cycles()
    s = side_stream()
    torch.cuda.synchronize()
    delay_done, done = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        delay_done.record(s)
        t0 = time.perf_counter()
        for k in b:
            b[k].copy_(staging[k])
        if call_on_default:
            with torch.cuda.stream(torch.cuda.default_stream()):
                res = case.call(b, o, ctx)
        else:
            res = case.call(b, o, ctx)
        ENQUEUE_MS[case.name] = (time.perf_counter() - t0) * 1e3
        done.record(s)
    still_running = not delay_done.query()
    s.synchronize()
    torch.cuda.synchronize()
    got = host_results(res)
    close(ctx)
    return got, still_running


def check_against_ref(case, got, want, where):
    bounds = want.get("_atol", {})
    for k, w in want.items():
        if k == "_atol":
            continue
        g, w = case.read(k, got[k]), np.asarray(w)
        assert g.shape == w.shape, (case.name, where, k, g.shape, w.shape)
        if k in bounds:
            assert (np.abs(g.astype(np.float64) - w.astype(np.float64)) <= bounds[k]).all(), (case.name, where, k, g, w)
        elif k in case.tol:
            rtol, atol = case.tol[k]
            np.testing.assert_allclose(g, w.astype(g.dtype), rtol=rtol, atol=atol, err_msg="%s %s %s" % (case.name, where, k))
        else:
            w = w.astype(g.dtype)
            if g.dtype.kind == "f":                   # any NaN equals any NaN (obs_ref.same_f64); everything else bit for bit
                assert np.array_equal(np.isnan(g), np.isnan(w)), (case.name, where, k)
                g, w = np.where(np.isnan(g), 0, g), np.where(np.isnan(w), 0, w)
            assert same_bits(g, w), "%s %s: %s differs from the CPU restatement" % (case.name, where, k)


def check_same(case, got, want, where):
    assert set(got) == set(want), (case.name, where)
    for k in want:
        assert same_bits(got[k], want[k]), "%s %s: %s differs from the default-stream run" % (case.name, where, k)


def host_inputs(b):
    return {k: host(v) for k, v in b.items()}


SEEDS_B = (1, 2, 3)                   # warm-up, replay 1, replay 2


def expected_sequence(case):
    """The three calls of part B made eagerly on the default stream, and the CPU restatement chained over them."""
    sets = [case.make(s) for s in SEEDS_B]
    b = {k: v.clone() for k, v in sets[0].items()}
    ctx = case.setup(SEEDS_B[0])
    eager, cpu, carried = [], [], None
    for i, cur in enumerate(sets):
        for k in b:
            if k not in case.state:
                b[k].copy_(cur[k])
        if case.ref is not None:
            h = host_inputs(b)
            if carried is not None:
                check_against_ref(case, h, carried, "state carried into call %d" % i)
            want = case.ref(h)
            carried = {k: want[k] for k in case.state + (("_atol",) if "_atol" in want else ())}
            cpu.append(want)
        res = case.call(b, sentinels(case), ctx)
        torch.cuda.synchronize()
        eager.append(host_results(res))
    close(ctx)
    return eager, cpu


def run_captured(case):
    """Part B, steps 1-3 -> host results after the warm-up (not compared), replay 1 and replay 2."""
    sets = [case.make(s) for s in SEEDS_B]
    ctx = case.setup(SEEDS_B[0])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    got = []
    with torch.cuda.stream(s):
        b = {k: v.clone() for k, v in sets[0].items()}
        o = sentinels(case)
        case.call(b, o, ctx)                                   # the eager warm-up: state now stands after set 0
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            res = case.call(b, o, ctx)
        for cur in sets[1:]:
            for k in b:
                if k not in case.state:
                    b[k].copy_(cur[k])
            for t in o.values():
                sentinel_(t)
            g.replay()
            s.synchronize()
            got.append(host_results(res))
    torch.cuda.synchronize()
    close(ctx)
    return got
