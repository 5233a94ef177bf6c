"""What test_minigrid_view_edges_gpu.py parametrises over against what csrc/minigrid_view.hip compiles (read from the
source, as test_engine_tables_cpu.py does for the engine): an instantiation added to the dispatch switch without a
test turns this file red.  Also, on the CPU oracle alone: the inputs of the GPU file meet the conditions that make
its comparisons meaningful, and the reward grid really separates Python's three roundings from a contracted fma."""
import glob
import os
import re
from fractions import Fraction

import numpy as np

import minigrid_view_oracle as mvo
import test_minigrid_view_edges_gpu as edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source():
    return open(glob.glob(os.path.join(ROOT, "goal-*_amd", "csrc", "minigrid_view.hip"))[0]).read()


def test_every_compiled_view_size_is_parametrised():
    src = _source()
    cases = re.findall(r"^\s*case (\d+): MG_LAUNCH_COLS\((\d+)\); break;", src, re.M)
    assert cases and all(a == b for a, b in cases)
    assert sorted(int(a) for a, _ in cases) == sorted(edges.COMPILED) and len(cases) == len(set(cases))
    assert len(re.findall(r"\bcase\b", src)) == len(cases)                 # no case line in another spelling
    assert len(re.findall(r"MG_LAUNCH_COLS\(\d+\)", src)) == len(cases)
    assert len(re.findall(r"default: MG_LAUNCH\(0\); break;", src)) == 1   # everything else: the runtime-V kernel
    header = open(os.path.join(ROOT, "include", "minigrid_view.h")).read()
    assert int(re.search(r"#define MG_MAX_VIEW (\d+)", header).group(1)) == edges.MAX_VIEW == max(edges.RUNTIME)
    assert sorted(edges.COMPILED + edges.RUNTIME) == list(range(1, edges.MAX_VIEW + 1))
    thr = re.search(r"const bool rows = \(size_t\)n_envs \* width \* height >= (\d+);", src)
    assert int(thr.group(1)) == edges.ROWS_MIN_BYTES
    assert all(W * H * N < edges.ROWS_MIN_BYTES for W, H, N in edges.BYTE_WORLDS)


def test_edge_inputs_meet_their_conditions():
    """The input conditions of sections a-c (hidden cells, spreading masks, directions, carried objects, door states)
    hold for every case; they depend on the oracle alone, so they are checked here without a GPU as well."""
    n = 0
    for st in (False, True):
        for V in edges.COMPILED:
            for W, H in edges.ROWS_WORLDS:
                edges.honest(edges.batch(W, H, edges.n_partial(V)), V, st)
                n += 1
            for W, H, N in edges.BYTE_WORLDS + [(8, 8, 1)]:
                edges.honest(edges.batch(W, H, N, edges.SALT.get((W, H, N), 0)), V, st)
                n += 1
        for V in edges.RUNTIME:
            for W, H in (edges.small_world(V), (17, 17)):
                edges.honest(edges.batch(W, H, edges.n_partial(V)), V, st)
                n += 1
        for V in edges.COMPILED + (6, 16, 31):
            edges.honest(edges.batch(5, 4, 80, agents="borders"), V, st)
            n += 1
    assert n == 2 * (8 * 10 + 23 * 2 + 11)
    shares = [edges.oracle(edges.batch(17, 17, edges.n_partial(V)), V, False)[1].mean() for V in (13, 15, 17)]
    assert all(0.05 < s < 0.6 for s in shares), shares                     # occlusion is neither absent nor total


def test_reward_grid_separates_python_rounding_from_a_contracted_fma():
    differ = at17 = 0
    for max_steps in range(1, 201):
        for step_count in range(1, max_steps + 1):
            q = step_count / max_steps
            fma = float(1 - Fraction(0.9) * Fraction(q))                   # one rounding, as v_fma_f64 would give
            differ += fma != 1 - 0.9 * q
            at17 += max_steps == 17 and fma != 1 - 0.9 * q
    assert differ > 20100 // 3 and at17 == 5, (differ, at17)              # a third of the grid; 5 of 17 at max_steps = 17
    assert mvo.step(mvo.Grid(3, 3), 0, 1, 0, 0, 17, 6)[6] == 0.0          # no goal, no reward
