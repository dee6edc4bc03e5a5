#!/usr/bin/env python3
"""McClendon difficulty / complexity of the hand-built tree mazes of tests/maze_shapes.py, from the
reference's own code: every maze of maze_shapes.cases() scored by ComplexityEvaluation(maze, start,
goal).difficulty_of_maze() / complexity_of_maze() (lib/maze_difficulty_evaluation/
maze_complexity_evaluation.py:38-329). The three generators never make these shapes (one corridor
through the whole maze, hallways of chosen sizes, trees off the odd lattice), so they pin the
hallway orders where generator mazes do not reach. Where the reference raises (neighbouring points
d = 0 apart: ZeroDivisionError; a start on the bottom or right border: IndexError) the values are
NaN; an overflow to inf is kept as the value.
Test infrastructure only (build container). Writes tests/golden/shapes.npz (data only: family
ids, sizes, padded grids, start / goal, values).
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main(ref="/root/reference"):
    import maze_shapes as S
    from make_golden import load_reference
    R = load_reference(ref)
    cs = S.cases()
    d = np.full(len(cs), np.nan)
    c = np.full(len(cs), np.nan)
    t0 = time.time()
    for i, m in enumerate(cs):
        g = [list(map(int, r)) for r in m["grid"]]
        try:
            ce = R["CE"](g, tuple(m["start"]), tuple(m["goal"]))
            d[i], c[i] = float(ce.difficulty_of_maze()), float(ce.complexity_of_maze())
        except (ZeroDivisionError, ValueError, IndexError) as e:
            print("  raises:", m["family"], m["name"], type(e).__name__, flush=True)
        print(i, m["family"], m["name"], d[i], round(time.time() - t0, 1), flush=True)
    pitch = max(m["n"] for m in cs)
    grids = np.zeros((len(cs), pitch, pitch), np.uint8)
    for i, m in enumerate(cs):
        grids[i, :m["n"], :m["n"]] = m["grid"]
    np.savez_compressed(
        os.path.join(HERE, "shapes.npz"),
        family=np.array([S.FAMILIES.index(m["family"]) for m in cs], np.uint8),
        n=np.array([m["n"] for m in cs], np.int32), grid=grids,
        start=np.array([m["start"] for m in cs], np.int32),
        goal=np.array([m["goal"] for m in cs], np.int32), difficulty=d, complexity=c)


if __name__ == "__main__":
    main(*sys.argv[1:])
