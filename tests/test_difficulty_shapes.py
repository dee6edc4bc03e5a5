"""The host McClendon restatement (mz_maze_complexity, csrc/mz_difficulty.hip) and the Python
oracle (oracle/mcclendon.py) on hand-built tree mazes: tests/golden/shapes.npz holds the
reference's ComplexityEvaluation values (maze_complexity_evaluation.py:310-329) of the mazes of
tests/maze_shapes.py — serpentines, spirals, combs, zig-zag teeth of chosen hallway sizes, binary,
Kruskal and Wilson trees, trees off the odd lattice, a leaf on the border — shapes the reference's
three generators, the source of every other fixture, do not make. CPU-only."""
import math

import numpy as np
import pytest

import maze_shapes as S
import shape_cases as SC


@pytest.fixture(scope="module")
def diff():
    from mazerl import difficulty
    from mazerl import _build
    _build.build()
    return difficulty


def test_builders_regenerate_the_fixture_grids():
    cs, ms = S.cases(), SC.mazes()
    assert len(cs) == len(ms) >= 150
    for c, m in zip(cs, ms):
        assert c["family"] == m["family"] and c["n"] == m["n"], m["index"]
        assert np.array_equal(c["grid"], m["grid"]), m["index"]
        assert tuple(c["start"]) == m["start"] and tuple(c["goal"]) == m["goal"], m["index"]


def test_fixture_covers_the_families_and_sizes():
    ms = SC.mazes()
    for fam in S.FAMILIES:
        sizes = {m["n"] for m in ms if m["family"] == fam}
        assert sizes and max(sizes) >= 80, (fam, sizes)  # every family has one at 81 (shifted: 80 / 81)
    assert sum(m["n"] <= 41 for m in ms) > len(ms) * 3 // 4
    for m in ms:  # bordered trees with a marked goal, as mz_load_mazes takes them
        g = m["grid"]
        assert g[m["goal"]] == 2 and g[m["start"]] == 1 and (g == 2).sum() == 1
        o = g != 0
        assert (o[:-1] & o[1:]).sum() + (o[:, :-1] & o[:, 1:]).sum() == o.sum() - 1, m["index"]
        assert S.open_border(g) == (m["family"] == "border")


def test_host_restatement_matches_the_reference_bit_for_bit(diff):
    n = 0
    for m in SC.mazes():
        if not SC.finite(m):
            continue
        d, c = diff.maze_complexity(m["grid"], m["start"], m["goal"])
        assert d == m["difficulty"] and c == m["complexity"], (m["index"], m["family"], m["n"])
        assert diff.maze_difficulty(m["grid"], m["start"], m["goal"]) == m["difficulty"]
        n += 1
    assert n >= 150


def test_host_restatement_reports_an_error_where_the_reference_raises(diff):
    """The fixture's NaN rows. The staircases: neighbouring points lie d = 0 apart and the
    reference's 1 / (2 d) raises ZeroDivisionError. A start on an open border square: its
    neighbour count indexes row / column -1 (Python's last one) or N (IndexError); the host reads
    no square outside the grid there (tests/sanitize/san_difficulty.cc runs the same case under
    AddressSanitizer). The host must not hand back a finite value."""
    rows = [m for m in SC.mazes() if not SC.finite(m)]
    assert len(rows) >= 8 and {m["family"] for m in rows} == {"staircase", "border"}
    for m in rows:
        try:
            d, c = diff.maze_complexity(m["grid"], m["start"], m["goal"])
        except (ValueError, RuntimeError):  # libmazerl's MZ_EINVAL
            continue
        assert not math.isfinite(d) and not math.isfinite(c), (m["n"], d, c)


def test_python_oracle_matches_the_reference_bit_for_bit():
    """Every maze of <= 41 squares and one 81-square maze per family."""
    M = SC.oracle()
    big, n = set(), 0
    for m in SC.mazes():
        if not SC.finite(m):
            continue
        if m["n"] > 41:
            if m["n"] < 81 or m["family"] in big:
                continue
            big.add(m["family"])
        assert M.evaluate(m["grid"], m["start"], m["goal"]) == (m["difficulty"], m["complexity"]), \
            (m["index"], m["family"], m["n"])
        n += 1
    assert big == set(S.FAMILIES) - {"staircase"} and n >= 150


def test_must_score_class_is_two_thirds_of_the_fixture_and_every_path_is_reached():
    """The class of mazes the GPU kernel has to score itself (tests/test_mcclendon_shapes_gpu.py),
    computed from the mazes and the oracle alone, and the kernel paths the fixture is built to
    reach ("Hand-built mazes")."""
    ms = SC.mazes()
    must = [m for m in ms if SC.finite(m) and SC.must_score(m["index"])]
    assert 3 * len(must) >= 2 * len(ms), (len(must), len(ms))
    f = [SC.facts(m["index"]) for m in ms]
    views = sorted({v for x in f for v in x["views"]})
    # phase G picks a hallway's path by its view size nc + nasp: <= 3 thread, <= 15 lane, else wave
    assert {2, 3, 4, 15, 16}.issubset(views), views
    # ... the set tables' resize points (5 and 20 entries, 64 .. 77 where a 128-slot table ends)
    assert {5, 6, 20, 21, 48, 63, 64, 77, 78, 79}.issubset(views), views
    mv = [x for m, x in zip(ms, f) if SC.finite(m) and SC.must_score(m["index"])]
    # ... a view holding at least half of the graph (iterated in G's node order), small and large
    assert any(x["half_view"] and x["view"] <= 15 for x in mv)
    assert any(x["half_view"] and x["view"] > 15 for x in mv)
    assert any(x["half_view"] and x["view"] > SC.VIEW_CAP for x in f)
    # ... each reason the kernel leaves a maze to the host for
    assert sum(x["goal_straight"] for x in f) >= 3 and sum(x["all_junctions"] for x in f) >= 3
    assert sum(x["open_border"] for x in f) >= 4 and sum(x["view"] > 63 for x in f) >= 2
    assert any(not x["odd_lattice"] and m["n"] % 2 == 1 for m, x in zip(ms, mv))
