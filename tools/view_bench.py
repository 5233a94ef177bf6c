#!/usr/bin/env python3
"""Throughput of the general MiniGrid view kernel (mg_gen_obs) and base step (mg_step) on random worlds.
Prints one JSON line per configuration: views/s and the HBM roofline fraction for the algorithmic bytes
(window cells of three planes read + image and mask written).

  python tools/view_bench.py [--envs 262144] [--size 17] [--iters 20]
  python tools/view_bench.py --obs [--obs_envs 4096]      the observation wrappers (minigrid_obs) instead: every kind at
                                                          view sizes 17 and 7, each beside a torch composition of the
                                                          same result and the fill_ rate of a buffer of its size; median
                                                          and range of --repeats windows of --obs_iters launches
  python tools/view_bench.py --nav [--obs_envs 4096]      the distance fields (minigrid_nav) on Twoarmy's 17x17 worlds: the
                                                          field, the agent's values alone and the lookup over T = 128
                                                          steps, beside a torch dilation loop that builds the same field
                                                          and the fill_ rate of each output size; windows as for --obs
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from twoarmy_amd import minigrid_view as mv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=262144)
ap.add_argument("--size", type=int, default=17)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--obs", action="store_true")
ap.add_argument("--nav", action="store_true")
ap.add_argument("--obs_envs", type=int, default=4096)
ap.add_argument("--obs_iters", type=int, default=200)
ap.add_argument("--repeats", type=int, default=9)
a = ap.parse_args()
dev = torch.device("cuda", 0)


def obs_rows():
    """One JSON line per (kind, view size, implementation)."""
    import statistics
    import torch.nn.functional as F
    from twoarmy_amd import minigrid_obs as mo
    N, S = a.obs_envs, 17
    g = torch.Generator(device="cpu").manual_seed(2)
    ty = torch.tensor([1, 1, 1, 1, 1, 2, 2, 6, 8], dtype=torch.uint8)[torch.randint(0, 9, (N, S * S), generator=g)].to(dev)
    co = torch.randint(0, 6, (N, S * S), generator=g, dtype=torch.uint8).to(dev)
    ax, ay, ad = (torch.randint(0, hi, (N,), generator=g, dtype=torch.int32).to(dev) for hi in (S, S, 4))
    tail = torch.from_numpy(mo.mission_tail("get to the green goal square")).to(dev)
    env_idx = torch.arange(N, device=dev)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.obs_iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.obs_iters * 1e3                         # us per call

    def row(kind, V, impl, fn, out_bytes, check=None):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        us = sorted(window(fn) for _ in range(a.repeats))
        med = statistics.median(us)
        print(json.dumps({"kind": kind, "view": V, "impl": impl, "envs": N, "out_MB": out_bytes / 1e6, "us_median": med,
                          "us_min": us[0], "us_max": us[-1], "store_GBs": out_bytes / med / 1e3, "equal": check}), flush=True)

    for V in (17, 7):
        img = torch.stack([ty[:, :V * V], co[:, :V * V], torch.zeros_like(ty[:, :V * V])], -1).view(N, V, V, 3).contiguous()
        long = img.long()
        oh = torch.empty((N, V, V, 21), dtype=torch.uint8, device=dev)
        comp = lambda: torch.cat([F.one_hot(long[..., 0], 12), F.one_hot(long[..., 1], 6), F.one_hot(long[..., 2], 3)], -1).to(torch.uint8)  # noqa: E731
        mo.onehot(img, out=oh)
        row("onehot", V, "mg_obs_onehot", lambda: mo.onehot(img, out=oh), oh.numel(), bool(torch.equal(oh, comp())))
        row("onehot", V, "torch one_hot+cat", comp, oh.numel())
        row("onehot", V, "torch fill_", lambda: oh.fill_(1), oh.numel())
        fl = torch.empty((N, V * V * 3 + tail.numel()), dtype=torch.float32, device=dev)
        compf = lambda: torch.cat([img.view(N, -1).float(), tail.expand(N, -1)], 1)                            # noqa: E731
        mo.flat_obs(img, tail, out=fl)
        row("flat", V, "mg_obs_flat", lambda: mo.flat_obs(img, tail, out=fl), fl.numel() * 4, bool(torch.equal(fl, compf())))
        row("flat", V, "torch float+cat", compf, fl.numel() * 4)
        row("flat", V, "torch fill_", lambda: fl.fill_(1), fl.numel() * 4)
    full = torch.empty((N, S, S, 3), dtype=torch.uint8, device=dev)
    stamp = torch.stack([torch.full_like(ad, 10), torch.zeros_like(ad), ad], -1).to(torch.uint8)

    def compfull():
        e = ty.view(N, S, S) <= 1
        o = torch.stack([torch.where(e, 1, ty.view(N, S, S)), torch.where(e, 0, co.view(N, S, S)), torch.zeros_like(e, dtype=torch.uint8)],
                        -1).permute(0, 2, 1, 3).contiguous()
        o[env_idx, ax.long(), ay.long()] = stamp
        return o
    mo.full_obs(ty, co, None, S, S, ax, ay, ad, out=full)
    row("full", S, "mg_obs_full", lambda: mo.full_obs(ty, co, None, S, S, ax, ay, ad, out=full), full.numel(),
        bool(torch.equal(full, compfull())))
    row("full", S, "torch where+permute+stamp", compfull, full.numel())
    sym = torch.empty((N, S, S, 3), dtype=torch.int32, device=dev)
    xs, ys = torch.meshgrid(torch.arange(S, device=dev, dtype=torch.int32), torch.arange(S, device=dev, dtype=torch.int32), indexing="ij")

    def compsym():
        t = ty.view(N, S, S).int()
        return torch.stack([xs.expand(N, S, S), ys.expand(N, S, S), torch.where(t <= 1, -1, t)], -1)
    mo.symbolic_obs(ty, S, S, out=sym)
    row("symbolic", S, "mg_obs_symbolic", lambda: mo.symbolic_obs(ty, S, S, out=sym), sym.numel() * 4, bool(torch.equal(sym, compsym())))
    row("symbolic", S, "torch where+stack", compsym, sym.numel() * 4)
    ty[:, 2 * S + 14] = 8
    k = mo.goal_index(ty, S, S)
    tab = mo.angle_table(S, S, dev)
    gd = torch.empty(N, dtype=torch.float64, device=dev)
    row("goal_index", S, "mg_obs_goal_index", lambda: mo.goal_index(ty, S, S), 4 * N)
    for mode in ("slope", "angle"):
        row("goal_direction " + mode, S, "mg_obs_goal_direction",
            lambda: mo.goal_direction(k, S, S, ax, ay, mode=mode, table=tab, out=gd), 8 * N)
    row("goal_direction slope", S, "torch div", lambda: (14 - ay).double() / (2 - ax).double(), 8 * N)
    row("goal_direction angle", S, "torch div+atan", lambda: torch.atan((14 - ay).double() / (2 - ax).double()), 8 * N)


def nav_rows():
    """One JSON line per (kind, implementation)."""
    import statistics
    from twoarmy_amd import minigrid_nav as nav
    from twoarmy_amd.engine import TwoarmyEngine
    N, S, T = a.obs_envs, 17, 128
    eng = TwoarmyEngine(4, N, 17, device=dev)
    eng.reset()
    ty = eng.plane_views()[0]
    agent = eng.agent_views()[:2]

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.obs_iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.obs_iters * 1e3                         # us per call

    def row(kind, impl, fn, out_bytes, check=None):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        us = sorted(window(fn) for _ in range(a.repeats))
        med = statistics.median(us)
        print(json.dumps({"kind": kind, "impl": impl, "envs": N, "out_MB": out_bytes / 1e6, "us_median": med, "us_min": us[0],
                          "us_max": us[-1], "store_GBs": out_bytes / med / 1e3, "equal": check}), flush=True)

    passable = torch.zeros(256, dtype=torch.bool, device=dev)
    passable[[t for t in range(16) if (nav.PASS_DEFAULT >> t) & 1]] = True

    def dilation():
        """The same field from whole-tensor ops: 4-neighbour dilation of the reached set until it stops changing (one
        host synchronisation per step, to see that it has)."""
        ok = passable[ty.long()].view(N, S, S)
        reached = (ty.view(N, S, S) == 8) & ok
        d = torch.where(reached, 0, nav.UNREACHABLE).to(torch.int32)
        k = 0
        while True:
            k += 1
            grown = reached.clone()
            grown[:, 1:] |= reached[:, :-1]
            grown[:, :-1] |= reached[:, 1:]
            grown[:, :, 1:] |= reached[:, :, :-1]
            grown[:, :, :-1] |= reached[:, :, 1:]
            fresh = grown & ok & ~reached
            if not bool(fresh.any()):
                return d.view(N, S * S)
            d = torch.where(fresh, k, d)
            reached |= fresh

    field = torch.empty((N, S * S), dtype=nav.DIST_DTYPE, device=dev)
    nav.distance_field(ty, None, S, S, out=field, want_error=False)
    same = bool(torch.equal(nav.as_int(field), dilation()))
    row("field 17x17", "mg_nav_field", lambda: nav.distance_field(ty, None, S, S, out=field, want_error=False),
        field.numel() * 2, same)
    row("field 17x17", "torch dilation loop", dilation, field.numel() * 2)
    row("field 17x17", "torch fill_", lambda: field.view(torch.int16).fill_(1), field.numel() * 2)
    ad, aa = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2))
    row("agent only", "mg_nav_field", lambda: nav.distance_field(ty, None, S, S, agent=agent, want_field=False,
                                                                 want_error=False, agent_out=(ad, aa)), 8 * N)
    row("agent only", "mg_nav_field, results allocated per call",
        lambda: nav.distance_field(ty, None, S, S, agent=agent, want_field=False, want_error=False), 8 * N)
    g = torch.Generator(device="cpu").manual_seed(3)
    pos = (torch.rand((T, N, 2), generator=g) * S).to(dev)
    out = torch.empty((T, N), dtype=nav.DIST_DTYPE, device=dev)
    nav.lookup(field, pos, S, S, out=out)
    want = nav.as_int(field)[torch.arange(N, device=dev), (pos[..., 0].long() * S + pos[..., 1].long())]
    row("lookup T=128", "mg_nav_lookup", lambda: nav.lookup(field, pos, S, S, out=out), out.numel() * 2,
        bool(torch.equal(nav.as_int(out), want)))
    row("lookup T=128", "torch gather", lambda: field.view(torch.int16)[torch.arange(N, device=dev),
                                                                        (pos[..., 0].long() * S + pos[..., 1].long())],
        out.numel() * 2)
    row("lookup T=128", "torch fill_", lambda: out.view(torch.int16).fill_(1), out.numel() * 2)
    eng.close()


if a.obs:
    obs_rows()
    sys.exit(0)
if a.nav:
    nav_rows()
    sys.exit(0)
N, W = a.envs, a.size
g = torch.Generator(device="cpu").manual_seed(1)
ty = torch.tensor([1, 1, 1, 1, 1, 2, 2, 4, 5, 6, 8], dtype=torch.uint8)[torch.randint(0, 11, (N, W * W), generator=g)].to(dev)
co = torch.randint(0, 6, (N, W * W), generator=g, dtype=torch.uint8).to(dev)
st = torch.where(ty == 4, torch.randint(0, 3, (N, W * W), generator=g, dtype=torch.uint8).to(dev), torch.zeros_like(ty))
ax = torch.randint(0, W, (N,), generator=g, dtype=torch.int32).to(dev)
ay = torch.randint(0, W, (N,), generator=g, dtype=torch.int32).to(dev)
d = torch.randint(0, 4, (N,), generator=g, dtype=torch.int32).to(dev)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.iters * 1e-3


for V, see in ((7, False), (7, True), (17, False), (17, True)):
    out = torch.empty((N, V, V, 3), dtype=torch.uint8, device=dev)
    s = timed(lambda: mv.gen_obs(ty, co, st, W, W, ax, ay, d, V, see, None, want_mask=False, out=out))
    nbytes = N * (3 * V * V + 3 * V * V + 12)
    print(json.dumps({"kernel": "mg_gen_obs", "envs": N, "world": "%dx%d" % (W, W), "view": V, "see_through_walls": see,
                      "ms": s * 1e3, "views_per_s": N / s, "algorithmic_GBs": nbytes / s / 1e9,
                      "frac_of_8TBs": nbytes / s / 8e12}), flush=True)
sc = torch.zeros(N, dtype=torch.int32, device=dev)
act = torch.randint(0, 4, (N,), generator=g, dtype=torch.int32).to(dev)
s = timed(lambda: mv.step(ty, st, W, W, act, ax, ay, d, sc, 1 << 30))
print(json.dumps({"kernel": "mg_step", "envs": N, "ms": s * 1e3, "steps_per_s": N / s}), flush=True)
