#!/usr/bin/env python3
"""Throughput of the device renderer (mg_render) on the Twoarmy engine's own state after a 64-step rollout.
One JSON line per configuration: ms per launch (HIP events over --iters launches after a warm-up), frames/s, GB/s on
the algorithmic bytes (frame written + two planes and the agent read) and that as a fraction of the 1 GiB `fill_` rate
of the same device taken in the same process (the yardstick of bench.py --full).

  python tools/render_bench.py [--envs 4096] [--iters 20]
  python tools/render_bench.py --pov           # mg_render_pov instead: the agents' 7 x 7 views at tile size 8
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from twoarmy_amd.engine import TwoarmyEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pov", action="store_true", help="time mg_render_pov (view size 7, tile size 8) instead of mg_render")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)

    def timed(fn):
        fn()
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters * 1e-3

    buf = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    fill = (1 << 30) / timed(lambda: buf.fill_(7))
    del buf
    print(json.dumps({"kernel": "fill_ 1 GiB", "GBs": fill / 1e9}), flush=True)
    eng = TwoarmyEngine(6, a.envs, 17, device=dev, seed=9981)
    out = eng.alloc_outputs(64)
    eng.rollout(64, out, actions=eng.fill_actions(64))
    g = torch.Generator(device="cpu").manual_seed(1)
    some = torch.randperm(a.envs, generator=g)[:16].to(dev, torch.int32)
    if a.pov:
        V, ts = 7, 8
        for idx in (None, some):
            n = a.envs if idx is None else idx.numel()
            frames = torch.empty((n, V * ts, V * ts, 3), dtype=torch.uint8, device=dev)
            s = timed(lambda: eng.render_pov(env_index=idx, tile_size=ts, view_size=V, out=frames))
            nbytes = n * (V * V * ts * ts * 3 + 2 * V * V + 12)          # frame written + the view's cells of two planes + agent
            print(json.dumps({"kernel": "mg_render_pov", "envs": a.envs, "frames": n, "view_size": V, "tile_size": ts,
                              "ms": s * 1e3, "frames_per_s": n / s, "algorithmic_GBs": nbytes / s / 1e9,
                              "frac_of_fill": nbytes / s / fill, "frac_of_8TBs": nbytes / s / 8e12}), flush=True)
            del frames
        eng.close()
        return
    for ts, idx, highlight in ((17, None, False), (17, None, True), (17, some, False), (32, None, False), (8, None, False)):
        n = a.envs if idx is None else idx.numel()
        frames = torch.empty((n, 17 * ts, 17 * ts, 3), dtype=torch.uint8, device=dev)
        s = timed(lambda: eng.render(env_index=idx, tile_size=ts, highlight=highlight, out=frames))
        nbytes = n * (289 * ts * ts * 3 + 578 + 12) + (a.envs * 289 * 2 if highlight else 0)
        print(json.dumps({"kernel": "mg_render", "envs": a.envs, "frames": n, "tile_size": ts, "highlight": highlight,
                          "ms": s * 1e3, "frames_per_s": n / s, "algorithmic_GBs": nbytes / s / 1e9,
                          "frac_of_fill": nbytes / s / fill, "frac_of_8TBs": nbytes / s / 8e12}), flush=True)
        del frames
    eng.close()


if __name__ == "__main__":
    main()
